"""Game records: what VecCatanEnv.recordings() hands back, how it is stored, replayed and printed.

A game's draws come from Philox keyed by (seed, global game id) and counted by the game's own draw counter, which is part of the state
blob (rng_draws).  A start blob, the applied actions, the seed, the game id and the env configuration therefore reproduce the game bit
for bit on a fresh one-game env: `replay` does exactly that, with product code only."""
import numpy as np

from . import spec

ACTION_TYPE_NAMES = ["PlaceSettlement", "PlaceRoad", "UpgradeToCity", "BuyDevelopmentCard", "PlayDevelopmentCard", "ExchangeResource",
                     "ProposeTrade", "RespondToOffer", "MoveRobber", "RollDice", "EndTurn", "StealResource", "DiscardResource"]
PLAYER_COLOURS = ["White", "Blue", "Orange", "Red"]                # PlayerId 1..4
CARD_NAMES = ["Knight", "VictoryPoint", "YearOfPlenty", "RoadBuilding", "Monopoly"]
T_ROLL, T_PLAYDEV = 9, 4
# slot states and flags of include/catan_hip_tuning.h
IDLE, WAIT_DEAL, RECORDING, SEALED = 0, 1, 2, 3
F_TRUNCATED, F_FROM_DEAL, F_GUARD_BROKEN = 1, 2, 4
RECORD_NOW, RECORD_AT_DEAL = 0, 1
# every catan_cfg_t field, as VecCatanEnv's keyword arguments take them (None: no limit)
CFG_FIELDS = ("max_proposed_trades_per_turn", "dense_reward", "validate_actions", "auto_reset", "win_reward", "reward_annealing_factor",
              "max_actions_per_turn")


class GameRecord(object):
    """One recorded game.  seed / game_id: the Philox key and the GLOBAL game id (env_id0 + the game's index).  cfg: dict of CFG_FIELDS,
    the reward annealing factor as it was when the slot was armed.  start_blob / final_blob: int32 [736] (final_blob None: the game
    was still being recorded).  actions: int32 [L, 18], L = min(length, capacity).  length: actions applied while recording;
    truncated: length exceeded the slot's capacity; from_deal: the start blob is a fresh deal (armed at_deal)."""

    def __init__(self, seed, game_id, cfg, start_blob, final_blob, actions, length, truncated=False, from_deal=False):
        self.seed, self.game_id = int(seed), int(game_id)
        self.cfg = {k: cfg[k] for k in CFG_FIELDS}
        self.start_blob = np.ascontiguousarray(start_blob, dtype=np.int32).reshape(spec.STATE_WORDS)
        self.final_blob = None if final_blob is None else np.ascontiguousarray(final_blob, dtype=np.int32).reshape(spec.STATE_WORDS)
        self.actions = np.ascontiguousarray(actions, dtype=np.int32).reshape(-1, spec.ACTION_WORDS)
        self.length, self.truncated, self.from_deal = int(length), bool(truncated), bool(from_deal)

    def __eq__(self, other):
        if not isinstance(other, GameRecord):
            return NotImplemented
        return ((self.seed, self.game_id, self.cfg, self.length, self.truncated, self.from_deal) ==
                (other.seed, other.game_id, other.cfg, other.length, other.truncated, other.from_deal)
                and np.array_equal(self.start_blob, other.start_blob) and np.array_equal(self.actions, other.actions)
                and (self.final_blob is None) == (other.final_blob is None)
                and (self.final_blob is None or np.array_equal(self.final_blob, other.final_blob)))

    __hash__ = None


def cfg_dict(c, reward_annealing_factor=None):
    """a _lib.CatanCfg -> the dict a GameRecord keeps (the two limits as VecCatanEnv takes them: None = no limit)"""
    return {"max_proposed_trades_per_turn": None if c.max_proposed_trades_per_turn < 0 else int(c.max_proposed_trades_per_turn),
            "dense_reward": bool(c.dense_reward), "validate_actions": bool(c.validate_actions), "auto_reset": bool(c.auto_reset),
            "win_reward": float(c.win_reward),
            "reward_annealing_factor": float(c.reward_annealing_factor if reward_annealing_factor is None else reward_annealing_factor),
            "max_actions_per_turn": None if c.max_actions_per_turn < 0 else int(c.max_actions_per_turn)}


def save(record, path):
    """.npz of arrays and scalars only (np.load(allow_pickle=False) reads it); a limit of None is stored as -1"""
    c = record.cfg
    lim = lambda v: np.int64(-1 if v is None else v)
    np.savez(path, format_version=np.int64(1), seed=np.uint64(record.seed), game_id=np.uint64(record.game_id),
             cfg_max_proposed_trades_per_turn=lim(c["max_proposed_trades_per_turn"]), cfg_dense_reward=np.bool_(c["dense_reward"]),
             cfg_validate_actions=np.bool_(c["validate_actions"]), cfg_auto_reset=np.bool_(c["auto_reset"]),
             cfg_win_reward=np.float64(c["win_reward"]), cfg_reward_annealing_factor=np.float64(c["reward_annealing_factor"]),
             cfg_max_actions_per_turn=lim(c["max_actions_per_turn"]),
             start_blob=record.start_blob, has_final=np.bool_(record.final_blob is not None),
             final_blob=record.final_blob if record.final_blob is not None else np.zeros((0,), dtype=np.int32),
             actions=record.actions, length=np.int64(record.length), truncated=np.bool_(record.truncated),
             from_deal=np.bool_(record.from_deal))


def load(path):
    with np.load(path, allow_pickle=False) as z:
        if int(z["format_version"]) != 1:
            raise ValueError(f"{path}: unknown game record format {int(z['format_version'])}")
        lim = lambda v: None if int(v) < 0 else int(v)
        cfg = {"max_proposed_trades_per_turn": lim(z["cfg_max_proposed_trades_per_turn"]), "dense_reward": bool(z["cfg_dense_reward"]),
               "validate_actions": bool(z["cfg_validate_actions"]), "auto_reset": bool(z["cfg_auto_reset"]),
               "win_reward": float(z["cfg_win_reward"]), "reward_annealing_factor": float(z["cfg_reward_annealing_factor"]),
               "max_actions_per_turn": lim(z["cfg_max_actions_per_turn"])}
        return GameRecord(int(z["seed"]), int(z["game_id"]), cfg, z["start_blob"], z["final_blob"] if bool(z["has_final"]) else None,
                          z["actions"], int(z["length"]), bool(z["truncated"]), bool(z["from_deal"]))


def _replay_env(record, device):
    from .env import VecCatanEnv
    c = record.cfg
    env = VecCatanEnv(1, seed=record.seed, env_id0=record.game_id, device=device,
                      max_proposed_trades_per_turn=c["max_proposed_trades_per_turn"], win_reward=c["win_reward"],
                      dense_reward=c["dense_reward"], validate_actions=c["validate_actions"], auto_reset=False,
                      max_actions_per_turn=c["max_actions_per_turn"])
    env.set_reward_annealing_factor(c["reward_annealing_factor"])
    return env


def replay(record, device=None, env=None):
    """Steps the record's actions from its start blob on a one-game VecCatanEnv made with seed = record.seed, env_id0 = record.game_id, the
    record's configuration and auto_reset = False.  Yields, per action, (step, deciding PlayerId, action int32 [18], reward float32 [4],
    done, blob int32 [736] after the action).  A truncated record replays the actions it holds.
    env: an env of that description to use instead (anything with import_state / deciding_player / step / export_state for ONE game)."""
    import torch
    if env is None:
        env = _replay_env(record, device)
    env.import_state(record.start_blob[None])
    for t in range(record.actions.shape[0]):
        who = int(env.deciding_player()[0])
        a = record.actions[t]
        reward, done = env.step(torch.from_numpy(a.copy()).view(1, spec.ACTION_WORDS))
        blob = env.export_state()[0]
        yield (t, who, a, np.array(reward[0].cpu().numpy(), dtype=np.float32), bool(int(done[0])),
               np.array(blob.cpu().numpy(), dtype=np.int32))


def _heads(a):
    """the head indices the action's type uses (env/wrapper.py:114-166 of the reference)"""
    t = int(a[spec.A_TYPE])
    if t in (0, 2):
        return f" corner {int(a[spec.A_CORNER])}"
    if t == 1:
        e = int(a[spec.A_EDGE])
        return " edge none" if e == spec.N_EDGES else f" edge {e}"
    if t == 8:
        return f" tile {int(a[spec.A_TILE])}"
    if t == 11:
        return f" target +{int(a[spec.A_PLAYER]) + 1}"                 # next / next-next / next-next-next player
    if t == T_PLAYDEV:
        card = int(a[spec.A_CARD])
        s = f" card {CARD_NAMES[card] if 0 <= card < 5 else card}"
        if card == 4:
            s += f" res {int(a[spec.A_RES_A])}"
        elif card == 2:
            s += f" res {int(a[spec.A_RES_A])},{int(a[spec.A_RES_B])}"
        return s
    if t == 5:
        return f" res {int(a[spec.A_RES_A])}->{int(a[spec.A_RES_B])}"
    if t == 6:
        give = [int(x) for x in a[spec.A_GIVE:spec.A_GIVE + 4]]
        recv = [int(x) for x in a[spec.A_RECV:spec.A_RECV + 4]]
        return f" target +{int(a[spec.A_PLAYER]) + 1} give {give} for {recv}"
    if t == 7:
        return " accept" if int(a[spec.A_RESPONSE]) == 0 else " reject"
    if t == 12:
        return f" res {int(a[spec.A_DISCARD])}"
    return ""


def describe_step(step, who, action, done, blob, before=None):
    """one line for one replayed action; before: the blob in front of it (an action that changed nothing was rejected)"""
    t = int(action[spec.A_TYPE])
    name = ACTION_TYPE_NAMES[t] if 0 <= t < len(ACTION_TYPE_NAMES) else f"type {t}"
    colour = PLAYER_COLOURS[who - 1] if 1 <= who <= 4 else f"player {who}"
    line = f"{step:5d} turn {int(spec.state_field(blob, 'turn')[0]):4d} {colour:6s} {name}{_heads(action)}"
    if before is not None and np.array_equal(before, blob):
        line += " (rejected)"
    elif t == T_ROLL:
        line += f" dice {int(spec.state_field(blob, 'die1')[0])}+{int(spec.state_field(blob, 'die2')[0])}"
    line += "  vp " + " ".join(str(int(v)) for v in spec.state_field(blob, "curr_vps"))
    if done:
        w = int(spec.state_field(blob, "winner")[0])
        line += f"  {PLAYER_COLOURS[w - 1] if 1 <= w <= 4 else w} wins"
    return line


def describe(record, device=None, env=None):
    """-> list of text lines: a header, then one line per action of the replay (step, turn, player colour, action-type name, the head
    indices the type uses, the dice of a roll, the four players' victory points after the action), and a note when the record is
    truncated."""
    lines = [f"game {record.game_id} seed {record.seed}: {record.length} actions"
             + (", from its deal" if record.from_deal else "") + (", still recording" if record.final_blob is None else "")]
    before = record.start_blob
    for step, who, a, _r, done, blob in replay(record, device, env):
        lines.append(describe_step(step, who, a, done, blob, before))
        before = blob
    if record.truncated:
        lines.append(f"truncated: the first {record.actions.shape[0]} of {record.length} actions were kept")
    return lines
