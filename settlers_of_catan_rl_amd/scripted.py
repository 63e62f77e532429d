"""The rule-based players as policy objects: the "builder" (csrc/catan_scripted.hip) and the "trader" (8.14;
csrc/catan_players.hip), which is the builder plus answers to offers, proposals and exchanges for a goal; and the playout player (8.15;
csrc/catan_players.hip), which picks among their moves and a few random ones by playing each out on the device.

A fixed-strength opponent: the same on every run and every checkpoint, far stronger than uniform-random play (DESIGN.md 8.8 has the
measured win share), one kernel launch per pass where a net's pass is a whole forward.  It sits wherever a net does - a seat of `evaluation.run_evaluation_episodes`, an opponent of
`rollout.RolloutCollector` - and reads the games themselves instead of their observations: the caller passes `games`, the row -> game
map of the pass (`wants_games`)."""
import torch

STYLES = ("builder", "trader")


class GamesPolicy(object):
    """A player that reads the games themselves: bound to an env, it answers a pass with int32 [rows, 18] actions.  A subclass supplies
    `_rows(env, games)`, the call that yields them."""
    wants_games = True            # the callers hand over which game each row of a pass is
    include_lstm = False

    def rebind(self, env):
        self.env = env
        return self

    def _bound_env(self):
        if self.env is None:
            name = type(self).__name__
            raise RuntimeError(f"{name} is not bound to an env ({name}(env) or rebind(env))")
        return self.env

    def _rows(self, env, games):
        raise NotImplementedError

    @torch.no_grad()
    def act(self, f, lists, lens, masks, games=None, deterministic=False, generator=None, **ignored):
        """-> (value zeros [rows,1], actions int64 [rows,18], log-prob zeros [rows,1]): the tuple acting.act's callers index.  The
        observation tensors only say how many rows the pass has; row j is game games[j] (None: game j, and the pass must then hold
        all of the env's games)."""
        env = self._bound_env()
        name = type(self).__name__
        rows = int(f.shape[0])
        if games is None:
            if rows != env.n:
                raise ValueError(f"{name}.act without `games` decides all {env.n} games of its env, the pass has {rows} rows")
        elif int(games.numel()) != rows:
            raise ValueError(f"{name}.act: {int(games.numel())} games for {rows} rows")
        a = self._rows(env, games).long()
        zeros = torch.zeros((rows, 1), dtype=torch.float32, device=a.device)
        return zeros, a, zeros.clone()

    @torch.no_grad()
    def label(self, games=None):
        """The player as a TEACHER -> int32 [rows, 18]: its action for game games[j] (None: every game), completed so
        that it can be teacher-forced through the net's heads (env.complete_action_rows)."""
        env = self._bound_env()
        return env.complete_action_rows(self._rows(env, games), games=games)


class ScriptedPolicy(GamesPolicy):
    """The rule-based player.  As a teacher, two launches; the trader's labels hold Propose rows and accepts."""
    default_style = "builder"

    def __init__(self, env=None, style=None):
        """env: the env whose games it decides (anything with `n` and `sample_scripted_actions(games=, style=)`: env.VecCatanEnv); None:
        unbound until `rebind` - the evaluation protocol binds it to the env of each call.  style: "builder" or "trader" (None: the
        class's own, "builder" here)."""
        style = self.default_style if style is None else style
        if style not in STYLES:
            raise ValueError(f"{type(self).__name__}: style must be one of {STYLES}, got {style!r}")
        self.env = env
        self.style = style

    def _rows(self, env, games):
        # (the builder's call is the one it always was: an env stand-in that knows no styles still serves it)
        return env.sample_scripted_actions(games=games) if self.style == "builder" else env.sample_scripted_actions(games=games, style=self.style)


class TraderPolicy(ScriptedPolicy):
    """ScriptedPolicy whose style defaults to "trader" (DESIGN.md 8.14): `run_evaluation_protocol(baselines={"trader": TraderPolicy})`,
    `RolloutCollector(opponents=[TraderPolicy(env)])`, `RolloutCollector(teacher=TraderPolicy(env))`."""
    default_style = "trader"


class RandomPolicy(GamesPolicy):
    """The uniform-random legal sampler (env.sample_random_actions) as a seat: the weakest fixed player, the floor of a rating scale.
    Every pass draws one action for every game of the env at the next step index (the number of passes since it was bound) and hands
    out the rows asked for: equal games and an equal pass number give equal actions."""

    def __init__(self, env=None):
        self.env, self.passes = env, 0

    def rebind(self, env):
        self.env, self.passes = env, 0
        return self

    def _rows(self, env, games):
        a = env.sample_random_actions(self.passes)
        self.passes += 1
        return a if games is None else a[games.long()]


class PlayoutPolicy(GamesPolicy):
    """The flat Monte-Carlo playout player (env.playout_actions): per decision it takes the builder's move, the trader's
    and `randoms` uniform-random legal ones, plays each out `playouts` times for `depth` env steps with the rule-based player of
    `playout_style` in every seat - on forked copies of the game in a scratch env of its own, re-dealt for what the deciding player cannot
    see if `determinise` - and plays the candidate with the best integer score (ties: the lowest index, i.e. the builder's move).  It needs
    no net and has ScriptedPolicy's interface: a seat of `evaluation.run_evaluation_episodes`, `run_evaluation_protocol(baselines={"playout":
    PlayoutPolicy})`, `RolloutCollector(opponents=[PlayoutPolicy(env)])`, `RolloutCollector(teacher=PlayoutPolicy(env))`.

    The defaults (randoms=2, playouts=8, depth=120) are defaults, not measured optima.  sim_games: the scratch env's games (None:
    candidates x playouts x min(env.n, 1024)); a pass with more rows than sim_games // (candidates x playouts) is decided in chunks.
    `step_idx` (the Philox index of the random candidates) goes up by one per call of the entry point - a chunked pass gives every chunk
    its own, since the chunks reuse the same scratch slots -: equal root states and an equal step_idx give equal bits.
    The root env must not be inside an open `step_deferred` sequence (the fork is refused there): `needs_lockstep` tells
    `RolloutCollector`, which then steps with `catan_step` (its default window becomes 0; an explicit window is refused)."""
    needs_lockstep = True             # it forks the env's games: not inside an open catan_step_deferred sequence (RolloutCollector steps lock-step for it)
    DEFAULT_SIM_ROWS = 1024
    SIM_ID_OFFSET = 1 << 40           # the scratch env's game ids start this far behind the root's: disjoint Philox streams

    def __init__(self, env=None, builder=True, trader=True, randoms=2, playouts=8, depth=120, playout_style="trader", determinise=True,
                 sim_games=None, seed=0):
        from . import spec
        name = type(self).__name__
        builder, trader, randoms, playouts, depth = int(bool(builder)), int(bool(trader)), int(randoms), int(playouts), int(depth)
        if randoms < 0 or not 1 <= builder + trader + randoms <= spec.PLAYOUT_MAX_CANDIDATES:
            raise ValueError(f"{name}: builder + trader + randoms must be in 1..{spec.PLAYOUT_MAX_CANDIDATES} (randoms >= 0), got {builder} + {trader} + {randoms}")
        if not 1 <= playouts <= spec.PLAYOUT_MAX_PLAYOUTS:
            raise ValueError(f"{name}: playouts must be in 1..{spec.PLAYOUT_MAX_PLAYOUTS}, got {playouts}")
        if depth < 1:
            raise ValueError(f"{name}: depth must be at least 1, got {depth}")
        if playout_style not in STYLES:
            raise ValueError(f"{name}: playout_style must be one of {STYLES}, got {playout_style!r}")
        self.candidates = (builder, trader, randoms)
        self.playouts, self.depth, self.playout_style, self.determinise = playouts, depth, playout_style, bool(determinise)
        per_row = sum(self.candidates) * playouts
        if sim_games is not None and int(sim_games) < per_row:
            raise ValueError(f"{name}: sim_games must hold at least one row's {per_row} playouts, got {sim_games}")
        self.sim_games = None if sim_games is None else int(sim_games)
        self.seed = int(seed)
        self.env = env
        self.sim = None
        self.step_idx = 0
        self.last_stats = self.last_chosen = None

    @property
    def sims_per_row(self):
        return sum(self.candidates) * self.playouts

    def rebind(self, env):
        if env is not self.env:
            self.sim = None            # the scratch env follows the root's limits and ids
        self.env = env
        return self

    def _make_sim(self, env, games):
        """-> the scratch env of `games` games for root `env`: no auto-reset, sparse reward, the root's turn and trade limits"""
        from .env import VecCatanEnv
        lim = lambda v: None if int(v) < 0 else int(v)
        return VecCatanEnv(games, seed=self.seed, env_id0=int(env.env_id0) + self.SIM_ID_OFFSET, device=env.device, auto_reset=False, dense_reward=False,
                           max_proposed_trades_per_turn=lim(env.cfg.max_proposed_trades_per_turn), max_actions_per_turn=lim(env.cfg.max_actions_per_turn))

    def _sim_for(self, env):
        if self.sim is None:
            games = self.sim_games if self.sim_games is not None else self.sims_per_row * min(int(env.n), self.DEFAULT_SIM_ROWS)
            self.sim = self._make_sim(env, games)
            self._sim_rows = games // self.sims_per_row
        return self.sim

    def _rows(self, env, games):
        """-> int32 [rows, 18]; fills last_stats / last_chosen; one call per chunk of the scratch env's rows"""
        sim = self._sim_for(env)
        rows, cap = int(env.n) if games is None else int(games.numel()), self._sim_rows
        kw = dict(candidates=self.candidates, playouts=self.playouts, depth=self.depth, playout_style=self.playout_style, determinise=self.determinise,
                  return_stats=True)
        first = self.step_idx
        if rows <= cap:
            self.step_idx += 1
            a, self.last_chosen, self.last_stats = env.playout_actions(sim, games, step_idx=first, **kw)
            return a.contiguous()
        g = torch.arange(rows, dtype=torch.int32, device=env.device) if games is None else games.reshape(-1)
        # every chunk runs in the same slots: its own step index keeps the chunks' random candidates on different Philox blocks
        parts = [env.playout_actions(sim, g[lo:lo + cap], step_idx=first + i, **kw) for i, lo in enumerate(range(0, rows, cap))]
        self.step_idx += len(parts)
        a, self.last_chosen, self.last_stats = (torch.cat([p[i] for p in parts], 0) for i in range(3))
        return a.contiguous()
