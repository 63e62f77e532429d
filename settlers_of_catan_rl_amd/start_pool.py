"""Start pools: saved positions that re-dealt games start from (VecCatanEnv.set_start_pool) - how a pool is held,
stored and harvested from game records or from a running env.

A pool entry is a state blob (int32 [736], the orientation of export_state).  Installed into a game it keeps the game's own draw
counter, so the same position in two games rolls different dice; the entry's own rng_draws word is therefore irrelevant and two
blobs that differ in it alone are the same position."""
import numpy as np

from . import spec


def _field(blob, name):
    return spec.state_field(blob, name)


def _position_key(blob):
    b = np.array(blob, dtype=np.int32, copy=True)
    _field(b, "rng_draws")[...] = 0
    return b.tobytes()


def leader_vp(blob):
    return int(max(int(v) for v in _field(blob, "curr_vps")))


class StartPool(object):
    """blobs int32 [m, 736]; per entry where it came from, int64 [m] each: seed, game_id (the GLOBAL id) and step (actions applied
    since the record's start blob), or -1 where that is unknown.
    Optional: weights, uint32 [m] - how often each entry is to be drawn relative to the others
    (VecCatanEnv.set_start_pool_weights) -, and outcomes, float64 [m + 1, 8] - the accumulated outcome tallies of the games started from each
    entry (columns spec.START_POOL_OUTCOME_FIELDS; the last row is the fresh deals'), multiplied by `decay` in front of every add_outcomes,
    as League.record does with its scoreboard.  decay = 1.0 (the default) keeps plain sums; like prior and floor of balanced_weights it is
    a hyper-parameter default and not a measured optimum."""

    def __init__(self, blobs, seed=None, game_id=None, step=None, weights=None, outcomes=None, decay=1.0):
        self.blobs = np.ascontiguousarray(blobs, dtype=np.int32).reshape(-1, spec.STATE_WORDS)
        m = len(self.blobs)
        col = lambda v, dt: np.full(m, -1, dtype=dt) if v is None else np.ascontiguousarray(v, dtype=dt).reshape(m)
        self.seed, self.game_id, self.step = col(seed, np.int64), col(game_id, np.int64), col(step, np.int64)
        self.weights = None if weights is None else _checked_weights(weights, m)
        self.outcomes = None if outcomes is None else np.array(outcomes, dtype=np.float64).reshape(m + 1, spec.START_POOL_OUTCOME_WORDS)
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"decay must be in [0, 1], got {decay}")
        self.decay = float(decay)

    def __len__(self):
        return len(self.blobs)

    def __eq__(self, other):
        if not isinstance(other, StartPool):
            return NotImplemented
        same = lambda a, b: (a is None) == (b is None) and (a is None or np.array_equal(a, b))
        return (all(np.array_equal(getattr(self, k), getattr(other, k)) for k in ("blobs", "seed", "game_id", "step"))
                and same(self.weights, other.weights) and same(self.outcomes, other.outcomes))

    def add_outcomes(self, table):
        """table: the tallies of one read - VecCatanEnv.start_pool_outcomes() (its "table") or an array [m + 1, 8].  What was accumulated
        so far is multiplied by `decay` first."""
        t = table["table"] if isinstance(table, dict) else table
        t = np.asarray(t, dtype=np.float64).reshape(len(self) + 1, spec.START_POOL_OUTCOME_WORDS)
        self.outcomes = t.copy() if self.outcomes is None else self.outcomes * self.decay + t

    def balanced_weights(self, prior=2.0, floor=1, scale=65535):
        """-> uint32 [m]: per entry p = (focus_wins + prior * 0.25) / (focus_games + prior) - 0.25 is a four-player game's fair share, so
        an entry never played has p = 0.25 - and weight = max(floor, round(scale * 4 * p * (1 - p))): the variance of the outcome, largest
        where the focus player wins half of the games, so that positions that are already decided are drawn less often.  prior and
        floor (and the pool's decay) are hyper-parameter defaults, not measured optima; no effect on training progress is claimed."""
        m = len(self)
        o = np.zeros((m + 1, spec.START_POOL_OUTCOME_WORDS)) if self.outcomes is None else self.outcomes
        games, wins = o[:m, spec.START_POOL_OUTCOME_FIELDS.index("focus_games")], o[:m, spec.START_POOL_OUTCOME_FIELDS.index("focus_wins")]
        den = games + float(prior)
        p = np.where(den > 0, (wins + float(prior) * 0.25) / np.where(den > 0, den, 1.0), 0.25)       # (prior = 0 and never played: the fair share)
        w = np.maximum(float(floor), np.round(float(scale) * 4.0 * p * (1.0 - p)))
        return _checked_weights(w.astype(np.int64), m)

    __hash__ = None

    def turns(self):
        return np.array([int(_field(b, "turn")[0]) for b in self.blobs], dtype=np.int64)

    def leader_vps(self):
        return np.array([leader_vp(b) for b in self.blobs], dtype=np.int64)

    def summary(self):
        """one line: entries, turn range, leader-VP histogram"""
        if not len(self):
            return "0 entries"
        t, v = self.turns(), self.leader_vps()
        hist = " ".join(f"{k}:{int((v == k).sum())}" for k in sorted(set(v.tolist())))
        return f"{len(self)} entries, turns {int(t.min())}..{int(t.max())}, leader VP {hist}"

    @classmethod
    def from_records(cls, records, every=1, skip_initial=True, min_turn=None, max_turn=None, min_leader_vp=None, max_leader_vp=None,
                     device=None, make_env=None):
        """Walks record.replay over every record and takes the position behind every `every`-th action (and the start blob) that passes
        the filters: skip_initial drops positions of the initial placement phase, min_ / max_turn bound the turn counter, min_ /
        max_leader_vp the leading player's points.  Finished positions are never taken; a position already in the pool (compared
        with rng_draws zeroed) is dropped.  make_env(record) -> the one-game env the replay runs on (default: record.replay's own)."""
        from . import record as _record
        if int(every) < 1:
            raise ValueError("every must be at least 1")
        blobs, seeds, ids, steps, seen = [], [], [], [], set()

        def consider(rec, step, blob):
            if int(_field(blob, "winner")[0]) != 0:
                return
            if skip_initial and int(_field(blob, "initial_phase")[0]) != 0:
                return
            turn, vp = int(_field(blob, "turn")[0]), leader_vp(blob)
            if (min_turn is not None and turn < min_turn) or (max_turn is not None and turn > max_turn):
                return
            if (min_leader_vp is not None and vp < min_leader_vp) or (max_leader_vp is not None and vp > max_leader_vp):
                return
            key = _position_key(blob)
            if key in seen:
                return
            seen.add(key)
            blobs.append(np.array(blob, dtype=np.int32)); seeds.append(rec.seed); ids.append(rec.game_id); steps.append(step)

        for rec in records:
            consider(rec, 0, rec.start_blob)
            env = None if make_env is None else make_env(rec)
            for t, _who, _a, _r, _done, blob in _record.replay(rec, device=device, env=env):
                if (t + 1) % int(every) == 0:
                    consider(rec, t + 1, blob)
        return cls(np.zeros((0, spec.STATE_WORDS), dtype=np.int32) if not blobs else np.stack(blobs), seeds, ids, steps)

    @classmethod
    def from_env(cls, env, games=None):
        """the current states of `games` (None: every game) that are unfinished; their origin is the env's seed and global ids"""
        idx = list(range(env.n)) if games is None else [int(g) for g in games]
        b = env.export_state() if games is None else env.export_state(idx)
        b = np.asarray(b.cpu().numpy() if hasattr(b, "cpu") else b, dtype=np.int32)
        keep = [j for j in range(len(idx)) if int(_field(b[j], "winner")[0]) == 0]
        return cls(b[keep], [env.seed] * len(keep), [env.env_id0 + idx[j] for j in keep], [-1] * len(keep))


def _checked_weights(weights, m):
    w = np.asarray(weights)
    if w.dtype.kind not in "iu" or w.shape != (m,):
        raise ValueError(f"weights: {m} integers expected, got {w.dtype} {tuple(w.shape)}")
    vals = [int(x) for x in w.tolist()]
    if any(x < 0 or x > 0xFFFFFFFF for x in vals) or (m and not 1 <= sum(vals) <= spec.START_POOL_MAX_WEIGHT_SUM):
        raise ValueError("weights must be in 0..2^32-1 and sum to 1..2^32-1")
    return np.array(vals, dtype=np.uint32).reshape(m)


def save(pool, path):
    """.npz of arrays only (np.load(allow_pickle=False) reads it); weights and outcomes (with the decay) only where the pool has them"""
    extra = {}
    if pool.weights is not None:
        extra["weights"] = pool.weights
    if pool.outcomes is not None:
        extra["outcomes"], extra["outcomes_decay"] = pool.outcomes, np.float64(pool.decay)
    np.savez(path, format_version=np.int64(1), blobs=pool.blobs, source_seed=pool.seed, source_game_id=pool.game_id, source_step=pool.step, **extra)


def load(path):
    with np.load(path, allow_pickle=False) as z:
        if int(z["format_version"]) != 1:
            raise ValueError(f"{path}: unknown start pool format {int(z['format_version'])}")
        names = set(z.files)
        return StartPool(z["blobs"], z["source_seed"], z["source_game_id"], z["source_step"],
                         weights=z["weights"] if "weights" in names else None, outcomes=z["outcomes"] if "outcomes" in names else None,
                         decay=float(z["outcomes_decay"]) if "outcomes_decay" in names else 1.0)
