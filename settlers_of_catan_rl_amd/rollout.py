"""Batched on-device rollout collection with the reference's active-seat bookkeeping.

Replaces `GamesAndPoliciesManager.gather_rollouts` / `_after_rollouts` / `reset` (reference RL/ppo/game_manager.py:35-59,
69-150) and the worker/pipe layer above it (RL/ppo/vec_gather_experience.py) by one lock-step device loop over all games:
every iteration encodes the observation of each game's deciding player (k_obs_rows), runs the policy of that seat, steps
all games (k_step) and updates the per-game bookkeeping with vectorised tensor ops.  Only the decisions of each game's
ACTIVE seat (the seat mapped to the central policy) are stored; rewards are accumulated across the other seats' moves.

The bookkeeping restates game_manager.py line by line (including its quirks, see comments) with four per-game counters
instead of Python lists: n_obs (observations), n_msk (terminal masks), n_act (actions / log-probs / action masks) and
n_rew (rewards).  A game is frozen (no-op actions) once it holds T+1 observations, until the slowest game catches up.
Storage is written directly in the `(T+1, N, ...)` layout of `BatchProcessor.process_rollouts`
(RL/ppo/process_batch.py:37-104), so no restacking is needed.

The env is duck-typed (`n`, `device`, `deciding_player`, `get_obs`, `get_action_masks`, `step` with auto-reset and
no-op for type < 0): `env.VecCatanEnv` on the GPU; the CPU tests use an oracle-backed stand-in.
"""
import torch

from . import _lib, acting, spec
from .env import _ptr, _stream


class RolloutStorage(object):
    """The tensors `BatchProcessor` holds after `process_rollouts` (process_batch.py:37-104), device resident."""
    _tokens = iter(range(1, 1 << 62))

    def invalidate(self):
        """the contents changed by other means than gather_rollouts (a loaded rollout, an in-place edit): consumers that cache
        per-rollout derived data (PPOTrainer's distinct boards) key on (token, generation) and recompute"""
        self.generation += 1

    def __init__(self, T, N, device, obs_dtype=torch.float32, lstm_size=0, teacher=False):
        self.T, self.N = T, N
        self.token = next(RolloutStorage._tokens)      # process-unique: a later storage at the same address is another rollout
        # process_batch.py:53-59: the active seat's LSTM state (h, c) entering each of its stored decisions
        self.hidden = torch.zeros((2, T + 1, N, lstm_size), dtype=torch.float32, device=device) if lstm_size else None
        self.obs_f = torch.zeros((T + 1, N, spec.OBS_FLOATS), dtype=obs_dtype, device=device)
        self.lists = torch.zeros((T + 1, N, 5, spec.OBS_LIST_PAD), dtype=torch.int8, device=device)
        self.lens = torch.ones((T + 1, N, 5), dtype=torch.int8, device=device)
        self.masks = torch.ones((T + 2, N), dtype=torch.float32, device=device)      # terminal masks (one spare slot, see reset quirk)
        self.rewards = torch.zeros((T + 2, N), dtype=torch.float32, device=device)
        self.actions = torch.zeros((T, N, spec.ACTION_WORDS), dtype=torch.int64, device=device)
        self.action_log_probs = torch.zeros((T, N), dtype=torch.float32, device=device)
        self.action_masks = torch.zeros((T, N, 11), dtype=torch.int32, device=device)   # packed 325-bit masks
        # RolloutCollector(teacher=...): the teacher's completed action row for every stored decision; allocated only then
        self.teacher_actions = torch.zeros((T, N, spec.ACTION_WORDS), dtype=torch.int16, device=device) if teacher else None
        self.games_complete = 0
        self.episode_stats = None     # RolloutCollector(episode_stats=True): the finished games of the last gather_rollouts (env.episode_stats)
        self.league_stats = None      # RolloutCollector(league_stats=True): their results per opponent net, int64 [nets + 1, 6] (env.league_stats)
        self.start_pool = None        # RolloutCollector(start_pool=...): the deals of the last gather_rollouts, {"pool", "fresh", "per_entry"} (env.start_pool_counts)
        self.records = None           # RolloutCollector(record_games=k): the games of the k record slots that ended in the last gather_rollouts (record.GameRecord)
        self.generation = 0           # bumped by every gather_rollouts (consumers cache per-rollout derived data on it)

    def unpack_action_masks(self, packed):
        """int32 [..., 11] -> float32 [..., 325]"""
        if packed.is_cuda and packed.dtype == torch.int32:            # one kernel (catan_expand_masks) instead of shift / and / slice / cast passes
            p = packed.contiguous()
            rows = p.numel() // p.shape[-1]
            out = torch.empty(packed.shape[:-1] + (spec.MASK_WORDS,), dtype=torch.float32, device=p.device)
            if rows == 0:                                             # an empty selection (empty minibatch / group): nothing to expand
                return out
            _lib.check(_lib.lib().catan_expand_masks(_ptr(p), rows, int(p.shape[-1]), _ptr(out), _stream()))
            return out
        bits = (packed[..., None] >> torch.arange(32, device=packed.device, dtype=torch.int32)) & 1
        return bits.reshape(packed.shape[:-1] + (352,))[..., :spec.MASK_WORDS].float()


def pack_action_masks(m):
    """float [N,325] -> int32 [N,11] (bit i of the flat mask -> word i>>5, bit i&31)"""
    N = m.shape[0]
    b = torch.zeros((N, 352), dtype=torch.int64, device=m.device)
    b[:, :spec.MASK_WORDS] = (m > 0).long()
    w = (b.reshape(N, 11, 32) << torch.arange(32, device=m.device)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).int()


def route_rows(pol, opp_index, n_opponents):
    """The net of each row of a league pass (0 = the central policy, 1 + k = opponent k) from the policy slot of its deciding seat (pol
    int64 [n]) and opp_index int64 [n, 3].  -> (order, counts): the rows sorted by net, ascending within a net (one stable sort), and
    the rows of each of the 1 + n_opponents nets (ONE host read per pass)."""
    ar = torch.arange(pol.shape[0], device=pol.device)
    net_id = torch.where(pol == 0, torch.zeros_like(pol), 1 + opp_index[ar, (pol - 1).clamp(min=0)])
    return torch.argsort(net_id, stable=True), torch.bincount(net_id, minlength=n_opponents + 1).tolist()


class _LaggedLiveCount(object):
    """(device loop) How many games still missed observations `lag` iterations ago: an upper bound of today's count (frozen games stay
    frozen) that costs no host wait per iteration - each one copies its count into a pinned ring and records an event."""

    def __init__(self, n, lag):
        self.lag, self.ring, self.bound = lag, lag + 2, n
        self.pin = torch.empty(self.ring, dtype=torch.int64).pin_memory()
        self.events = [torch.cuda.Event() for _ in range(self.ring)]

    def read(self, iters):
        j = iters - self.lag
        if j >= 1:
            self.events[j % self.ring].synchronize()
            self.bound = int(self.pin[j % self.ring])
        return self.bound

    def post(self, iters, count):
        self.pin[iters % self.ring].copy_(count, non_blocking=True)
        self.events[iters % self.ring].record()


class _PassRows(object):
    """(device loop) The rows of the policy pass: all N games, then - once the games that still miss observations fit a smaller captured
    bucket - the list of them as of that bucket change (a game that has frozen since just gets the no-op); row j is game games[j]."""

    def __init__(self, N):
        self.N, self.B, self.cnt = N, N, N           # games; rows of the captured pass; rows of it in use
        self.games = self.games_l = None             # the listed games as int32 (the env's kernels) and int64 (index_copy_); None: all
        self.inputs = None                           # GraphedAct.input_rows of this bucket, once the env writes into them
        self.full = None                             # (actions, logp) with one row per game

    def shrink(self, newB, live_now, sel):
        """-> whether the live games fit newB rows (ONE nonzero: the host read of a bucket change); then they are the list.  A game that
        froze since the count was taken would lose its last observation's append if this iteration's catan_obs_rows left it out: sel stays."""
        games_l = (live_now | sel.bool()).nonzero(as_tuple=True)[0]
        if games_l.numel() > newB:
            return False
        self.games_l, self.games, self.cnt, self.B = games_l, games_l.to(torch.int32).contiguous(), int(games_l.numel()), newB
        self.inputs = None                           # (the previous bucket's)
        if self.full is None:
            self.full = (sel.new_zeros((self.N, spec.ACTION_WORDS), dtype=torch.int64), sel.new_zeros((self.N,), dtype=torch.float32))
        return True

    def one_per_game(self, actions, logp):
        """a pass's rows scattered back to one row per game (the games outside the list are frozen: no-ops)"""
        if self.games is None:
            return actions, logp
        self.full[0].index_copy_(0, self.games_l, actions)
        self.full[1].index_copy_(0, self.games_l, logp)
        return self.full


class RolloutCollector(object):
    GRAPH_ACT_MIN_GAMES = 8192

    def __init__(self, env, policy, num_steps, opponents=None, seed=0, autocast_dtype=None, graph_act=None, deferred_window=None, act_buckets=None,
                 episode_stats=False, league_stats=False, record_games=0, start_pool=None, start_pool_fresh=0.0,
                 start_pool_outcomes=False, start_pool_sampling="uniform", teacher=None):
        """policy: central net (policy 0); opponents: list of up to 3 nets for policy slots 1..3 of every game (None =
        every seat plays the central policy).  A league (league.League.assign) installs per-game opponents instead.  An opponent
        may be a `scripted.ScriptedPolicy(env)` bound to this env: a fixed anchor beside the nets (its rows' log-probs are 0 and,
        like every opponent's, never stored).
        deferred_window: step the env with catan_step_deferred (window of that many iterations) instead of catan_step - the
        reference's workers advance every env independently (game_manager.py:78-113), and so do the games here: one whose step
        needs the slow path waits for it while the others go on (device collector only; 0 = catan_step; None = 4 where the env
        has the call: measured at 65 536 games x T = 200, tools/rollout_schedules.py: 2.50 s with catan_step, 2.44 s with W = 4).
        act_buckets: row counts of the captured policy passes (graph_act): once the games that still miss observations fit a
        smaller bucket, only they are evaluated (None = N, N/2, ... N/16 with graph_act, else N only).
        episode_stats: the env counts its finished games on the device (VecCatanEnv.enable_episode_stats, the active seat as the focus
        player); every gather_rollouts leaves the dict of the games that finished during it in storage.episode_stats - one read after
        the loop, none inside it.
        league_stats: the env also counts, per opponent net, who won the finished games (VecCatanEnv.enable_league_stats with this
        collector's seat map and the opponent indices of set_opponents, which re-enables it - between rollouts, behind the read); every
        gather_rollouts leaves the table, a row per net in the order of set_opponents' `nets` and a totals row, in storage.league_stats
        (None while no opponent is installed).  The same single read after the loop.
        record_games: games 0..k-1 are recorded whole, each from its next deal (VecCatanEnv.enable_recording / arm_recording(at_deal=True));
        every gather_rollouts leaves the games that ended during it in storage.records (record.GameRecord: replay, describe) and arms
        their slots again.  Read after the loop, like the statistics; the env needs auto_reset.
        start_pool: saved positions (a start_pool.StartPool, or blobs [m, 736]) that the env's re-dealt games start from, except for the
        share start_pool_fresh of deals, which stay fresh (VecCatanEnv.set_start_pool: installed here, in front of this collector's
        reset(); the games the env holds at that moment are not touched - env.reset() deals them from the pool).  Every gather_rollouts
        leaves the counts of its deals in storage.start_pool, read once after the loop like the statistics.  None: no call is made.
        start_pool_outcomes: the env also tallies the finished games by the pool entry they started from, the active seat as the focus
        player (VecCatanEnv.enable_start_pool_outcomes); every gather_rollouts leaves them in storage.start_pool["outcomes"], read once
        beside the counts.  start_pool_sampling "balanced" (implies the outcomes): behind every rollout the tallies are added to the
        pool (StartPool.add_outcomes; self.start_pool) and the entries' weights for the next rollout become its balanced_weights() - the
        positions whose result is still open are drawn more often.  The defaults (False, "uniform") make no call.
        teacher (kickstarting): any object with `label(games=None) -> int32 [N, 18]`, completed action rows for the
        deciding player of every game - `scripted.ScriptedPolicy(env)` is the one shipped.  Every env iteration labels all N games once,
        after the masks are read and before the step, and the label of a game goes into storage.teacher_actions (int16 [T, N, 18],
        allocated only with a teacher) at the slot its active seat's action goes into storage.actions; opponent seats are never
        labelled, nothing else in the storage changes.  `stop_teacher()` later stops the labelling and frees the tensor (train with
        teacher_coef 0 from then on).  The tensor-operation loop steps with catan_step whatever `deferred_window` says, with a
        teacher as without.  Not with LSTM policies.  None: no call is made.
        A teacher or opponent with `needs_lockstep` (scripted.PlayoutPolicy) makes the default deferred_window 0 (_honour_lockstep_players)."""
        self.env,self.policy, self.T = env, policy, num_steps
        self.league_stats, self.policy_of_pid = bool(league_stats), None
        self.deferred_window = self.DEFAULT_DEFERRED_WINDOW if deferred_window is None else int(deferred_window)
        self._window_given = deferred_window is not None
        self.teacher = None
        self.act_buckets = None if act_buckets is None else tuple(sorted(set(int(b) for b in act_buckets) | {env.n}))
        self.N, self.device = env.n, env.device
        if torch.device(self.device).type == "cuda":
            from . import nn_kernels
            nn_kernels.use_tuned_gemms()
        self.autocast_dtype = autocast_dtype
        self.opponent_nets, self.opp_index, self._graphed_nets = [], None, {}
        if opponents:
            nets = list(opponents)
            self.set_opponents(nets, torch.tensor([[min(j, len(nets) - 1) for j in range(3)]]).expand(self.N, 3))
        # acting nets under autocast hold their weights in the autocast dtype (policy.inference_copy): no per-call casts
        self._shadow = policy.inference_copy(autocast_dtype) if (autocast_dtype is not None and hasattr(policy, "inference_copy")) else None
        g = torch.Generator(device="cpu").manual_seed(seed)
        # game_manager.py:24-31: a random seat order per game; order[0] is the active player, order[j] plays policy j
        perm = torch.stack([torch.randperm(4, generator=g) for _ in range(self.N)])        # [N,4] pid0 per policy slot
        self.policy_of_pid = torch.empty((self.N, 4), dtype=torch.int64)
        self.policy_of_pid.scatter_(1, perm, torch.arange(4).expand(self.N, 4))
        self.policy_of_pid = self.policy_of_pid.to(self.device)
        self.active_pid = (perm[:, 0] + 1).long().contiguous().to(self.device)                                  # PlayerId 1..4
        self.sample_gen = torch.Generator(device=self.device).manual_seed(seed + 1)
        self.recurrent = bool(getattr(policy, "include_lstm", False))
        # Self-play with one feed-forward net: the policy pass of an env iteration is ~500 small launches and host-bound
        # (7.0 ms of host time for 5.3 ms of kernels at 65 536 rows) - replayed as one captured hipGraph instead
        # (acting.GraphedAct; sampling draws from the same registered generator).  graph_act: None = automatic.
        if graph_act is None:
            graph_act = (torch.device(self.device).type == "cuda" and not self.recurrent and hasattr(policy, "refresh_kernel_packs")
                         and self.N >= self.GRAPH_ACT_MIN_GAMES)
        self.graph_act, self._graphed = bool(graph_act), None
        self.lstm_size = int(policy.lstm_size) if self.recurrent else 0
        # Under autocast the net casts its inputs to the autocast dtype before the first GEMM anyway, and every observation
        # value is a small multiple of 1/8 (exact in bf16): the rollout tensors are kept in that dtype - half the HBM
        # (config 3: 58 instead of 116 GB) and no cast pass per minibatch.
        obs_dtype = autocast_dtype if (autocast_dtype in (torch.bfloat16, torch.float16) and torch.device(self.device).type == "cuda") else torch.float32
        if teacher is not None and self.recurrent:
            raise ValueError("RolloutCollector(teacher=...) is not supported with LSTM policies")
        if teacher is not None and not hasattr(teacher, "label"):
            raise ValueError("RolloutCollector(teacher=...): a teacher has label(games=None) -> int32 [N, 18] (scripted.ScriptedPolicy(env))")
        self.teacher = teacher
        self._honour_lockstep_players()
        self.storage = RolloutStorage(num_steps, self.N, self.device, obs_dtype=obs_dtype, lstm_size=self.lstm_size, teacher=teacher is not None)
        # game_manager.py:94-95 sums the env's rewards (Python floats) over the other seats' moves and process_batch.py:63
        # rounds the sum to fp32: the env leaves its unrounded rewards in a float64 buffer for that
        self.reward64 = env.enable_reward64() if hasattr(env, "enable_reward64") else None
        self.episode_stats = bool(episode_stats)
        if self.episode_stats:
            env.enable_episode_stats(self.active_pid)
        self._enable_league_stats()
        self.record_games = int(record_games)
        if self.record_games:
            env.enable_recording(list(range(self.record_games)))
            env.arm_recording(at_deal=True)
        self.install_start_pool(start_pool, start_pool_fresh, start_pool_outcomes, start_pool_sampling)
        self.reset()

    def install_start_pool(self, pool, fresh_share=0.0, outcomes=False, sampling="uniform"):
        """The one place that puts a start pool on the env, for the constructor's start_pool arguments and for TrainingLoop (TrainArgs'):
        `pool` as the constructor takes it, or the path of a saved pool; then the outcomes and, under "balanced", the first weights.
        None makes no call.  The games the env holds are not touched: the caller resets."""
        if sampling not in ("uniform", "balanced"):
            raise ValueError(f"start_pool_sampling must be 'uniform' or 'balanced', got {sampling!r}")
        if (outcomes or sampling != "uniform") and pool is None:
            raise ValueError("start_pool_outcomes / start_pool_sampling need a start_pool")
        self.start_pool_on, self.start_pool_sampling = pool is not None, sampling
        self.start_pool_outcomes = bool(outcomes) or sampling == "balanced"
        self.start_pool = None
        if pool is None:
            return
        from . import start_pool as _start_pool
        if isinstance(pool, str):
            pool = _start_pool.load(pool)
        self.env.set_start_pool(getattr(pool, "blobs", pool), fresh_share)
        if self.start_pool_outcomes:
            self.start_pool = pool if isinstance(pool, _start_pool.StartPool) else _start_pool.StartPool(pool)
            self.env.enable_start_pool_outcomes(self.active_pid)
            if sampling == "balanced":
                self.env.set_start_pool_weights(self.start_pool.balanced_weights())

    def stop_teacher(self):
        """No more labels from here on: the teacher goes and storage.teacher_actions (472 MB at 65 536 games x T = 200) is freed."""
        self.teacher = None
        if self.storage is not None:
            self.storage.teacher_actions = None

    def set_opponents(self, nets, opp_index):
        """nets: the distinct opponent nets in play; opp_index int64 [N,3]: which of them plays policy slots 1..3 of
        each game (game_manager.py:15,28-31: the slot -> seat map of a game stays fixed)."""
        self._graphed_nets = {}                  # (captured per-net passes belong to the nets they were captured with)
        # (a policy that reads the games themselves - scripted.ScriptedPolicy, bound to this collector's env - has no weights to copy)
        self.opponent_nets = [n.inference_copy(self.autocast_dtype) if (self.autocast_dtype is not None and hasattr(n, "inference_copy")
                                                                        and not getattr(n, "wants_games", False)
                                                                        and getattr(n, "_inference_dtype", None) is None) else n for n in nets]
        self.opp_index = opp_index.to(self.device).long().contiguous() if len(self.opponent_nets) else None
        self._honour_lockstep_players()
        self._enable_league_stats()

    def _honour_lockstep_players(self):
        """A teacher or an opponent with `needs_lockstep` (scripted.PlayoutPolicy: it forks the env's games, which an open
        catan_step_deferred sequence forbids) makes the collector step with catan_step from here on: deferred_window becomes 0 where it
        was left to the default, and a window asked for by the caller is refused.  The rollouts are the same either way."""
        who = [p for p in [self.teacher] + list(self.opponent_nets) if getattr(p, "needs_lockstep", False)]
        if not who or not self.deferred_window:
            return
        if self._window_given:
            raise ValueError(f"RolloutCollector: {type(who[0]).__name__} needs lock-step steps (it forks the env's games, which an open "
                             f"catan_step_deferred sequence forbids): deferred_window must be 0 or None, got {self.deferred_window}")
        self.deferred_window = 0

    def _enable_league_stats(self):
        """league_stats: the table for the opponents now installed, zeroed (called by set_opponents; the constructor calls it once its
        seat map exists)"""
        if not self.league_stats or self.policy_of_pid is None:
            return
        self._league_on = self.opp_index is not None
        if self._league_on:
            self.env.enable_league_stats(self.policy_of_pid, self.opp_index, len(self.opponent_nets))
        elif hasattr(self.env, "enable_league_stats"):
            self.env.enable_league_stats(None, None, 0, on=False)

    # game_manager.py:35-59 (the env itself is already reset: EnvWrapper.reset() happened in catan_create / env.reset())
    def reset(self):
        N, dev, st = self.N, self.device, self.storage
        # the four counters are rows of one tensor (and only ever updated in place): catan_collector_post takes them as one block
        self._cnt = torch.zeros((4, N), dtype=torch.int64, device=dev)
        self.n_obs, self.n_msk, self.n_act, self.n_rew = self._cnt[0], self._cnt[1], self._cnt[2], self._cnt[3]
        self.n_msk.fill_(1)                                                                 # terminal_masks = [1.0]
        self._flags = torch.zeros((4, N), dtype=torch.uint8, device=dev)                    # done_since, pending_obs, live, sel of the fused bookkeeping
        st.masks[0] = 1.0
        self.pending_obs = self.env.deciding_player().long() == self.active_pid             # observations = [obs] iff the active seat moves first
        self.done_since = torch.zeros(N, dtype=torch.bool, device=dev)
        self.racc = torch.zeros((N, 4), dtype=torch.float64, device=dev)
        if self.recurrent:            # game_manager.py:54-59: every seat of every game starts from the zero state
            self.hid = torch.zeros((2, N, 4, self.lstm_size), dtype=torch.float32, device=dev)

    # ---- "append to this game's list" for all games at once.  The selected games are never compacted on the host (a
    # `nonzero` is a device-to-host read of how many there are: five of them per env iteration kept the host from running
    # ahead, and the GPU idle while the host launched the next policy pass): big rows go through catan_masked_row_store,
    # per-game scalars through a read-modify-write of the whole column.
    def _row_store(self, dst, src, t, sel):
        """dst[t[n], n] = src[n] where sel[n]; dst [steps, N, ...], src [N, ...] (same trailing shape and dtype)"""
        if dst.is_cuda and hasattr(self.env, "L"):
            src = src.contiguous()
            row_bytes = src[0].numel() * src.element_size()
            _lib.check(_lib.lib().catan_masked_row_store(_ptr(dst), _ptr(src), _ptr(t), _ptr(sel), self.N, row_bytes, dst.stride(0) * dst.element_size(), _stream()))
            return
        idx = sel.nonzero(as_tuple=True)[0]
        if idx.numel():
            dst[t[idx], idx] = src[idx]

    def _col_store(self, dst, value, t, sel):
        """dst[t[n], n] = value[n] (or a scalar) where sel[n]; t in range for every n"""
        ar = self._ar
        cur = dst[t, ar]
        v = value if torch.is_tensor(value) else torch.full_like(cur, value)
        m = sel if cur.dim() == 1 else sel.reshape((-1,) + (1,) * (cur.dim() - 1))
        dst[t, ar] = torch.where(m, v.to(cur.dtype), cur)

    def _store_obs(self, sel, f, lists, lens, t=None):
        """f is None: the observation rows were already appended by the env (catan_obs_rows); only the bookkeeping is left"""
        st, T = self.storage, self.T
        if t is None:
            t = self.n_obs.clamp(max=T)
        sel8 = sel.to(torch.uint8)
        if f is not None:
            self._row_store(st.obs_f, f.to(st.obs_f.dtype), t, sel8)
            self._row_store(st.lists, lists.to(torch.int8), t, sel8)
            self._col_store(st.lens, lens.to(torch.int8), t, sel)
        if self.recurrent:            # game_manager.py:55,133: the state the active seat will enter this decision with
            hid = self.hid[:, self._ar, self.active_pid - 1]                                  # [2, N, L]
            for k in range(2):
                self._row_store(st.hidden[k], hid[k], t, sel8)
        self.n_obs += sel.long()

    fused_bookkeeping = True   # False: the tensor-operation form of the bookkeeping below (what the kernels are tested against)
    CHECK_EVERY = 8      # (tensor-operation form) env iterations between two host reads of "every game has its T + 1 observations"
    DEFAULT_DEFERRED_WINDOW = 4
    LIVE_LAG = 2         # (device collector) the host looks at the live-game count of this many iterations ago: no host wait per iteration

    def _group_buckets(self):
        """row counts of the captured per-net passes of a league rollout: a net's share of the games is about a quarter"""
        N = self.N
        return tuple(sorted({max(1024, N * k // 16) for k in (1, 2, 3, 4, 5, 6, 8, 12, 16)}))

    def _bucket_list(self):
        if self.act_buckets is not None:
            return self.act_buckets
        N = self.N
        if not self.graph_act:
            return (N,)
        halves = {N >> k for k in range(0, 6) if (N >> k) >= 1024}
        return tuple(sorted(halves | {3 * (b >> 2) for b in halves if 3 * (b >> 2) >= 1024}))      # N, 3N/4, N/2, 3N/8, ...

    @torch.no_grad()
    def gather_rollouts(self, max_iters=None):
        """game_manager.py:69-140.  Returns the storage (first T(+1) entries per game are the rollout)."""
        env, st, N, dev = self.env, self.storage, self.N, self.device
        try:
            self._ar = torch.arange(N, device=dev)
            if self._shadow is not None:
                self._shadow.load_from(self.policy)  # the central policy as of this rollout (game_manager.py:161-162 `_update_policy`)
            self.racc.zero_()                        # `rewards = {...: 0}` at the start of every gather call (:76)
            self.done_since.zero_()                  # `done_since_prev_turn = [False ...]` (:77)
            term = st.masks[0].clone()               # `terminal_mask = terminal_masks[env_num][0]` (:74-75)
            n_live_iters = torch.zeros((), dtype=torch.int64, device=dev)       # iterations in which some game still stepped
            n_complete = torch.zeros((), dtype=torch.int64, device=dev)
            # one kernel writes the dense observations the policy pass reads (in the storage's dtype: every value is exact in bf16)
            # AND appends the active seats' rows to the storage (k_obs_rows)
            fused_obs = hasattr(env, "get_obs_rows") and st.obs_f.is_cuda and st.obs_f.dtype in (torch.float32, torch.bfloat16)
            # ... and two kernels do the per-game bookkeeping of an iteration (catan_collector_pre / _post) instead of ~40 tensor operations
            if fused_obs and hasattr(env, "get_action_masks_packed") and not self.recurrent and hasattr(env, "L") and self.fused_bookkeeping:
                iters = self._gather_device(max_iters, term, n_live_iters, n_complete)
            else:
                iters = self._gather_tensor(max_iters, term, n_live_iters, n_complete, fused_obs)
            st.games_complete += int(n_complete)
            if self.episode_stats:
                st.episode_stats = env.episode_stats(reset=True)
            if self.league_stats:
                st.league_stats = env.league_stats(reset=True) if self._league_on else None
            if self.start_pool_on:
                st.start_pool = env.start_pool_counts(reset=True)
                if self.start_pool_outcomes:
                    st.start_pool["outcomes"] = env.start_pool_outcomes(reset=True)
                    if self.start_pool_sampling == "balanced":
                        self.start_pool.add_outcomes(st.start_pool["outcomes"])
                        env.set_start_pool_weights(self.start_pool.balanced_weights())
            if self.record_games:
                from . import record as _record
                sealed = (env.recording_status()[:, 0] == _record.SEALED).nonzero(as_tuple=True)[0].tolist()
                st.records = env.recordings(slots=sealed) if sealed else []
                if sealed:
                    env.arm_recording(slots=sealed, at_deal=True)
            st.generation += 1
            self.iters = int(n_live_iters) if max_iters is None else iters
            return st
        except BaseException:
            # an error inside the loop (a policy that raises, out of memory) must not leave a catan_step_deferred sequence open:
            # every later step / reset / export of the env would be refused until someone flushed it
            if self.deferred_window and hasattr(env, "step_flush"):
                try:
                    env.step_flush()
                except Exception:
                    pass
            raise

    def _gather_device(self, max_iters, term, n_live_iters, n_complete):
        """catan_obs_rows, the policy pass, catan_collector_pre, the env step, catan_collector_post; no host wait but the lagged count"""
        env, st, T, N, dev = self.env, self.storage, self.T, self.N, self.device
        fl = self._flags
        fl[0].copy_(self.done_since)
        fl[1].copy_(self.pending_obs)
        live8, sel_next = fl[2], fl[3]
        t_next = torch.empty(N, dtype=torch.int64, device=dev)
        a_env = torch.empty((N, spec.ACTION_WORDS), dtype=torch.int32, device=dev)
        deferred = bool(self.deferred_window) and hasattr(env, "step_deferred")
        stat, sk = (torch.zeros((2, N), dtype=torch.uint8, device=dev) if deferred else None), 0     # status of the previous / of this catan_step_deferred call (alternating)
        buckets = self._bucket_list() if ((self.graph_act or self.act_buckets is not None) and not self.opponent_nets and not self.recurrent) else (N,)
        rows, live = _PassRows(N), _LaggedLiveCount(N, self.LIVE_LAG)
        self.bucket_log = []         # (iteration, rows of the policy pass, listed games) at every bucket change of this rollout
        storage_rows = (st.obs_f, st.lists, st.lens)
        # which games append an observation where: afterwards written by catan_collector_post, which also counts the appends in n_obs
        sel, t_obs = self.pending_obs & (self.n_obs < T + 1), self.n_obs.clamp(max=T)
        iters = 0
        while True:
            bound = live.read(iters)
            newB = next(b for b in buckets if b >= max(bound, 1))
            if newB < rows.B and bound and rows.shrink(newB, self.n_obs < T + 1, sel):
                self.bucket_log.append((iters, rows.B, rows.cnt))
            f, lists, lens = env.get_obs_rows(st.obs_f.dtype, out=None if rows.inputs is None else rows.inputs[:3], rows=storage_rows, t=t_obs, sel=sel, games=rows.games)
            if iters == 0:
                self.n_obs += sel.long()
            if bound == 0 or (max_iters is not None and iters >= max_iters):
                break
            iters += 1
            deciding = env.deciding_player()                                                # :79
            masks = env.get_action_masks(None if rows.inputs is None else rows.inputs[3], games=rows.games)  # :83
            pol = self.policy_of_pid[self._ar, deciding.long() - 1] if self.opponent_nets else None
            actions, logp = self._act(f, lists, lens, masks, pol, games=rows.games)         # :85-89
            if rows.inputs is None and self._graphed is not None and not self.opponent_nets:
                # once the pass of this bucket is captured the env writes straight into its input buffers (no copy per replay)
                rows.inputs = self._graphed.input_rows(rows.B, rows.cnt, st.obs_f.dtype)
            actions, logp = rows.one_per_game(actions, logp)
            actions, logp = actions.contiguous(), logp.contiguous()
            _lib.check(_lib.lib().catan_collector_pre(N, T, _ptr(self.n_obs), _ptr(actions), _ptr(a_env), _ptr(live8), _stream()))
            n_live_iters += live8.any()
            pmasks = env.get_action_masks_packed()                                          # (before the step replaces them)
            labels = self.teacher.label().contiguous() if self.teacher is not None else None   # (the teacher reads the games before the step too)
            if deferred:
                wb, so = stat[sk], stat[sk ^ 1]
                reward, done, _ = env.step_deferred(a_env, self.deferred_window, status_out=so)
                sk ^= 1
            else:
                wb = so = None
                reward, done = env.step(a_env)                                              # :91 (auto-reset == :113)
            if labels is not None:       # in front of catan_collector_post: the slot is n_act BEFORE its increment
                _lib.check(_lib.lib().catan_collector_label(N, T, _ptr(self._cnt), _ptr(fl), _ptr(self.active_pid), _ptr(deciding), _ptr(labels),
                                                            _ptr(st.teacher_actions), _ptr(wb), _stream()))
            self._collector_post(term, t_next, n_complete, deciding, env.deciding_player(), actions, logp, pmasks, reward, done, wb, so)
            live.post(iters, (self.n_obs < T + 1).sum())
            sel, t_obs = sel_next, t_next
        if deferred:
            # the steps that are still outstanding (none when every game has frozen; some after `max_iters`): completed by the flush,
            # their results booked as in the loop, the observations they make the active seat's appended.  Every game counts as having
            # waited (`ones`): no decision is appended, none of deciding / actions / logp / pmasks read - the storage's tensors stand in
            reward, done, so = env.step_flush()
            ones = torch.ones(N, dtype=torch.uint8, device=dev)
            deciding = env.deciding_player()
            self._collector_post(term, t_next, n_complete, deciding, deciding, st.actions, st.action_log_probs, env.get_action_masks_packed(), reward, done, ones, so)
            env.get_obs_rows(st.obs_f.dtype, rows=storage_rows, t=t_next, sel=sel_next, dense=False)
        # (the loop left after an observation append: sel / pending_obs of the flags are consumed)
        self.done_since = fl[0].bool()
        self.pending_obs = torch.zeros(N, dtype=torch.bool, device=dev)
        return iters

    def _collector_post(self, term, t_next, n_complete, deciding, n_deciding, actions, logp, pmasks, reward, done, waiting_before, status):
        """catan_collector_post (include/catan_hip.h): books an env step's results and leaves in flags[3] / t_next which games append their
        next observation where.  waiting_before / status: of the previous / of this catan_step_deferred call, None with catan_step."""
        st = self.storage
        _lib.check(_lib.lib().catan_collector_post(
            self.N, self.T, _ptr(self._cnt), _ptr(self.racc), _ptr(self._flags), _ptr(term), _ptr(t_next), _ptr(self.active_pid), _ptr(deciding),
            _ptr(n_deciding), _ptr(actions), _ptr(logp), _ptr(pmasks), _ptr(reward), _ptr(self.reward64), _ptr(done), _ptr(st.actions),
            _ptr(st.action_log_probs), _ptr(st.action_masks), _ptr(st.rewards), _ptr(st.masks), _ptr(n_complete), _ptr(waiting_before), _ptr(status), _stream()))

    def _gather_tensor(self, max_iters, term, n_live_iters, n_complete, fused_obs):
        """what the device loop's kernels are tested against; the only form for the CPU oracle env, LSTM policies, fused_bookkeeping = False"""
        env, st, T, N, dev = self.env, self.storage, self.T, self.N, self.device
        inp = None               # the captured policy pass's input buffers, once the env writes into them
        iters = 0
        while True:
            if fused_obs:
                sel, t_obs = self.pending_obs & (self.n_obs < T + 1), self.n_obs.clamp(max=T)
                f, lists, lens = env.get_obs_rows(st.obs_f.dtype, out=None if inp is None else inp[:3], rows=(st.obs_f, st.lists, st.lens), t=t_obs, sel=sel)
                self._store_obs(sel, None, None, None, t=t_obs)
            else:
                f, lists, lens = env.get_obs()
                # an observation produced by the previous step for the active seat (:126-133) - or the carried one
                self._store_obs(self.pending_obs & (self.n_obs < T + 1), f, lists, lens)
            self.pending_obs = torch.zeros(N, dtype=torch.bool, device=dev)
            frozen = self.n_obs >= T + 1                                                    # while len(observations) < T+1 (:78)
            if (max_iters is not None and iters >= max_iters) or (iters % self.CHECK_EVERY == 0 and bool(frozen.all())):
                break
            iters += 1
            live = ~frozen
            n_live_iters += live.any()
            deciding = env.deciding_player().long()                                         # :79
            masks = env.get_action_masks(inp[3]) if inp is not None else env.get_action_masks()   # :83
            pol = self.policy_of_pid[self._ar, deciding - 1]
            actions, logp = self._act(f, lists, lens, masks, pol, deciding, term, live)     # :85-89
            if fused_obs and inp is None and self._graphed is not None and not self.opponent_nets:
                inp = self._graphed.input_rows(N, N, st.obs_f.dtype)                        # (as in the device loop)
            a_env = actions.to(torch.int32)
            a_env[:, 0] = torch.where(frozen, torch.full_like(a_env[:, 0], -1), a_env[:, 0])   # frozen games: no-op
            pmasks = env.get_action_masks_packed() if hasattr(env, "get_action_masks_packed") else pack_action_masks(masks)   # (before the step replaces them)
            labels = self.teacher.label() if self.teacher is not None else None             # (the teacher reads the games before the step too)
            reward, done = env.step(a_env)                                                  # :91 (auto-reset == :113)
            term = self._book_step(term, n_complete, live, deciding, actions, logp, pmasks, reward, done, labels)
        return iters

    def _book_step(self, term, n_complete, live, deciding, actions, logp, pmasks, reward, done, labels=None):
        """game_manager.py:91-136 for the games that stepped (`live`), as tensor operations.  -> the new terminal masks."""
        env, st, T, ar = self.env, self.storage, self.T, self._ar
        done = done.bool() & live
        term = torch.where(live, 1.0 - done.float(), term)                              # :97
        self.racc += (reward.double() if self.reward64 is None else self.reward64) * live[:, None]   # :94-95
        was_active = (deciding == self.active_pid) & live                               # :102-105
        t = self.n_act.clamp(max=T - 1)
        self._col_store(st.actions, actions, t, was_active)
        self._col_store(st.action_log_probs, logp, t, was_active)
        self._col_store(st.action_masks, pmasks, t, was_active)
        if labels is not None:
            self._col_store(st.teacher_actions, labels, t, was_active)
        self.n_act += was_active.long()
        n_deciding = env.deciding_player().long()                                       # after the step (and the reset)
        next_active = (n_deciding == self.active_pid) & live
        r_active = self.racc[ar, self.active_pid - 1]
        # :106-110 (not done: uses the post-step deciding player) and :112-118 (done: exactly one reward is appended)
        app = torch.where(done, torch.ones_like(done), next_active & (self.n_act > 0) & ~self.done_since) & live
        self._col_store(st.rewards, r_active.float(), self.n_rew.clamp(max=T + 1), app)        # process_batch.py:63
        self.n_rew += app.long()
        self.racc[ar, self.active_pid - 1] = torch.where(app, torch.zeros_like(r_active), r_active)
        # :112-124
        self._col_store(st.masks, 0.0, self.n_msk.clamp(max=T + 1), done)
        self.n_msk += done.long()
        self.done_since = self.done_since & ~done
        self.racc = torch.where(done[:, None], torch.zeros_like(self.racc), self.racc)
        if self.recurrent:
            self.hid = torch.where(done[None, :, None, None], torch.zeros_like(self.hid), self.hid)   # :121-124
        n_complete += done.sum()
        # :128-136
        add_mask = next_active & ~done & ~self.done_since
        self._col_store(st.masks, 1.0, self.n_msk.clamp(max=T + 1), add_mask)
        self.n_msk += add_mask.long()
        self.done_since = torch.where(next_active, torch.zeros_like(self.done_since),
                                      torch.where(done & live, torch.ones_like(self.done_since), self.done_since))
        self.pending_obs = next_active
        return term

    def _act(self, f, lists, lens, masks, pol, deciding=None, term=None, live=None, games=None):
        """One batched forward per distinct net in play: net 0 = central policy, net 1 + k = opponent_nets[k].
        With an LSTM policy the deciding seat's state goes in (multiplied by the previous step's terminal mask, :81,85-89)
        and its new state is kept for the games that really step."""
        N = f.shape[0]
        central = self.policy if self._shadow is None else self._shadow
        if not self.opponent_nets:
            groups = [(None, central)]
        else:
            order, counts = route_rows(pol, self.opp_index, len(self.opponent_nets))
            groups = [(idx, net) for idx, net in zip(order.split(counts), [central] + self.opponent_nets) if idx.numel()]
        actions = torch.zeros((N, spec.ACTION_WORDS), dtype=torch.int64, device=f.device)
        logp = torch.zeros((N,), dtype=torch.float32, device=f.device)
        if self.recurrent:
            ar_all = torch.arange(N, device=f.device)
            seat = deciding - 1
            h_in, c_in = self.hid[0, ar_all, seat], self.hid[1, ar_all, seat]
            new_h, new_c = h_in.clone(), c_in.clone()
        for idx, net in groups:
            args = (f, lists, lens, masks) if idx is None else (f[idx], lists[idx], lens[idx], masks[idx])
            kw = {"generator": self.sample_gen}
            if getattr(net, "wants_games", False) and (games is not None or idx is not None):
                # policies keyed by game (scripted.ScriptedPolicy, test policies): row j of this call is game games[j] - of the pass's
                # list, or of the net's share of the rows
                kw["games"] = games if idx is None else (idx if games is None else games[idx])
            if self.recurrent:
                sel = slice(None) if idx is None else idx
                kw.update(hidden=(h_in[sel], c_in[sel]), nonterminal=term[sel])
            res = self._call_net(net, args, kw, idx is None)
            if self.recurrent:
                new_h[sel], new_c[sel] = res[3][0].float(), res[3][1].float()
            if idx is None:
                actions, logp = res[1], res[2][:, 0]
            else:
                actions[idx] = res[1]
                logp[idx] = res[2][:, 0]
        if self.recurrent:
            keep = live[:, None]
            self.hid[0, ar_all, seat] = torch.where(keep, new_h, h_in)                     # :89
            self.hid[1, ar_all, seat] = torch.where(keep, new_c, c_in)
        return actions, logp

    def _call_net(self, net, args, kw, all_rows):
        """net.act for one group of rows: with graph_act a captured pass (same generator, registered with every graph) - the self-play
        pass over all rows, or a league net's share of them (one captured pass per net in play and bucket instead of ~150 host-bound
        launches; the rows beyond the group are padding) -, else the eager call."""
        if not (self.graph_act and not self.recurrent and (all_rows or (not getattr(net, "wants_games", False) and hasattr(net, "refresh_kernel_packs")))):
            return acting.act(net, args, self.autocast_dtype, **kw)
        g = self._graphed if all_rows else self._graphed_nets.get(id(net))
        if g is None or g.policy is not net:
            g = acting.GraphedAct(net, buckets=self._bucket_list() if all_rows else self._group_buckets(), autocast_dtype=self.autocast_dtype, generator=self.sample_gen)
            if all_rows:
                self._graphed = g
            else:
                self._graphed_nets[id(net)] = g
        return g(*args, with_logp=True, clone=False)

    def close(self):
        """Drops what the collector holds on the device - the captured policy passes (hipGraphs and their pools), the acting copy of
        the net and the rollout storage - without waiting for the garbage collector; the collector cannot be used afterwards."""
        for g in ([] if self._graphed is None else [self._graphed]) + list(self._graphed_nets.values()):
            g.graphs.clear()
        self._graphed = self._shadow = self.storage = None
        self._graphed_nets = {}
        self.opponent_nets = []

    # game_manager.py:142-150
    def after_rollouts(self):
        st, T, N = self.storage, self.T, self.N
        ar = torch.arange(N, device=self.device)
        last_t = (self.n_obs - 1).clamp(min=0)
        st.obs_f[0] = st.obs_f[last_t, ar]
        st.lists[0] = st.lists[last_t, ar]
        st.lens[0] = st.lens[last_t, ar]
        st.masks[0] = st.masks[(self.n_msk - 1).clamp(min=0, max=T + 1), ar]
        if self.recurrent:
            st.hidden[:, 0] = st.hidden[:, last_t, ar]
        had_obs = self.n_obs > 0
        self.n_obs.copy_(had_obs.long())
        self.n_msk.fill_(1)
        self.n_act.zero_()
        self.n_rew.zero_()
