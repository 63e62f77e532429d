"""The rule-based "builder" player as a policy object (csrc/catan_scripted.hip).

A fixed-strength opponent: the same on every run and every checkpoint, far stronger than uniform-random play (DESIGN.md 8.8 has the
measured win share), one kernel launch per pass where a net's pass is a whole forward.  It sits wherever a net does - a seat of `evaluation.run_evaluation_episodes`, an opponent of
`rollout.RolloutCollector` - and reads the games themselves instead of their observations: the caller passes `games`, the row -> game
map of the pass (`wants_games`)."""
import torch


class ScriptedPolicy(object):
    wants_games = True            # the callers hand over which game each row of a pass is
    include_lstm = False

    def __init__(self, env=None):
        """env: the env whose games it decides (anything with `n` and `sample_scripted_actions(games=)`: env.VecCatanEnv); None:
        unbound until `rebind` - the evaluation protocol binds it to the env of each call."""
        self.env = env

    def rebind(self, env):
        self.env = env
        return self

    @torch.no_grad()
    def act(self, f, lists, lens, masks, games=None, deterministic=False, generator=None, **ignored):
        """-> (value zeros [rows,1], actions int64 [rows,18], log-prob zeros [rows,1]): the tuple acting.act's callers index.  The
        observation tensors only say how many rows the pass has; row j is game games[j] (None: game j, and the pass must then hold
        all of the env's games)."""
        env = self.env
        if env is None:
            raise RuntimeError("ScriptedPolicy is not bound to an env (ScriptedPolicy(env) or rebind(env))")
        rows = int(f.shape[0])
        if games is None:
            if rows != env.n:
                raise ValueError(f"ScriptedPolicy.act without `games` decides all {env.n} games of its env, the pass has {rows} rows")
        elif int(games.numel()) != rows:
            raise ValueError(f"ScriptedPolicy.act: {int(games.numel())} games for {rows} rows")
        a = env.sample_scripted_actions(games=games).long()
        zeros = torch.zeros((rows, 1), dtype=torch.float32, device=a.device)
        return zeros, a, zeros.clone()

    @torch.no_grad()
    def label(self, games=None):
        """The player as a TEACHER -> int32 [rows, 18]: its action for game games[j] (None: every game), completed so
        that it can be teacher-forced through the net's heads (env.complete_action_rows).  Two launches."""
        env = self.env
        if env is None:
            raise RuntimeError("ScriptedPolicy is not bound to an env (ScriptedPolicy(env) or rebind(env))")
        return env.complete_action_rows(env.sample_scripted_actions(games=games), games=games)

