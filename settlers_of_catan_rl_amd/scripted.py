"""The rule-based players as policy objects: the "builder" (csrc/catan_scripted.hip) and the "trader" (8.14;
csrc/catan_trader.hip), which is the builder plus answers to offers, proposals and exchanges for a goal.

A fixed-strength opponent: the same on every run and every checkpoint, far stronger than uniform-random play (DESIGN.md 8.8 has the
measured win share), one kernel launch per pass where a net's pass is a whole forward.  It sits wherever a net does - a seat of `evaluation.run_evaluation_episodes`, an opponent of
`rollout.RolloutCollector` - and reads the games themselves instead of their observations: the caller passes `games`, the row -> game
map of the pass (`wants_games`)."""
import torch

STYLES = ("builder", "trader")


class ScriptedPolicy(object):
    wants_games = True            # the callers hand over which game each row of a pass is
    include_lstm = False
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

    def rebind(self, env):
        self.env = env
        return self

    def _sample(self, env, games):
        # (the builder's call is the one it always was: an env stand-in that knows no styles still serves it)
        return env.sample_scripted_actions(games=games) if self.style == "builder" else env.sample_scripted_actions(games=games, style=self.style)

    @torch.no_grad()
    def act(self, f, lists, lens, masks, games=None, deterministic=False, generator=None, **ignored):
        """-> (value zeros [rows,1], actions int64 [rows,18], log-prob zeros [rows,1]): the tuple acting.act's callers index.  The
        observation tensors only say how many rows the pass has; row j is game games[j] (None: game j, and the pass must then hold
        all of the env's games)."""
        env = self.env
        name = type(self).__name__
        if env is None:
            raise RuntimeError(f"{name} is not bound to an env ({name}(env) or rebind(env))")
        rows = int(f.shape[0])
        if games is None:
            if rows != env.n:
                raise ValueError(f"{name}.act without `games` decides all {env.n} games of its env, the pass has {rows} rows")
        elif int(games.numel()) != rows:
            raise ValueError(f"{name}.act: {int(games.numel())} games for {rows} rows")
        a = self._sample(env, games).long()
        zeros = torch.zeros((rows, 1), dtype=torch.float32, device=a.device)
        return zeros, a, zeros.clone()

    @torch.no_grad()
    def label(self, games=None):
        """The player as a TEACHER -> int32 [rows, 18]: its action for game games[j] (None: every game), completed so
        that it can be teacher-forced through the net's heads (env.complete_action_rows).  Two launches.  The trader's labels hold
        Propose rows and accepts (8.14)."""
        env = self.env
        name = type(self).__name__
        if env is None:
            raise RuntimeError(f"{name} is not bound to an env ({name}(env) or rebind(env))")
        return env.complete_action_rows(self._sample(env, games), games=games)


class TraderPolicy(ScriptedPolicy):
    """ScriptedPolicy whose style defaults to "trader" (DESIGN.md 8.14): `run_evaluation_protocol(baselines={"trader": TraderPolicy})`,
    `RolloutCollector(opponents=[TraderPolicy(env)])`, `RolloutCollector(teacher=TraderPolicy(env))`."""
    default_style = "trader"
