"""Generates tests/golden/board_configs.npz - board layouts (the reference Board's randomise_number_placement,
fixed_terrain_placements and fixed_number_order knobs, game/components/board.py:23-47,67-100) - by driving the imported upstream
reference through tools/ref_harness.py (development container only).  The fixture is DATA: layouts, actions, blobs, CRCs.

The reference's constructor check cannot run (np.array_equal with one argument, board.py:37-42, raises TypeError for either
fixed knob), so the layout is installed by substituting game.game.Board with a thin subclass that sets the three attributes
and then resets: EnvWrapper() and Game() draw in their usual order, Board.reset applies the layout exactly as it is written.

  layouts            L x (randomise, has_terrain, terrain[19], has_numbers, numbers[18]):
                     0 fixed terrain only, 1 fixed numbers only, 2 both (two touching reds), 3 randomise_number_placement=False
  reset_blobs        [L][S][P] post-reset blobs under the philox contract: seed SEEDS[s], env_id 100 + P * l + p
  traj{k}_*          philox trajectories of random legal steps with auto-reset on layout TRAJ_LAYOUT[k]: per step the state
                     crc, a crc of the packed masks, rewards, done; the actions; the final blob
  mt_*               the UNPATCHED reference (np.random.seed(s); random.seed(s); Board substituted with layout 3, which the real
                     constructor also accepts) - actions and per-step state crcs (rng word zeroed), the final blob
"""
import os
import random
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402
import game.game as ref_game  # noqa: E402  (reference)
from game.enums import Terrain  # noqa: E402  (reference)

from settlers_of_catan_rl_amd import spec  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "board_configs.npz")
SEEDS = (5, 77, 1234)
PAIRS = 16                      # env ids per (layout, seed)
TRAJ_LAYOUT = (2, 0)
TRAJ_SEEDS = ((9, 3), (13, 40))     # (seed, env_id)
TRAJ_STEPS = 5200
MT_SEED, MT_STEPS = 4, 4200

# a fixed terrain (row by row, tile ids 0..18 as in board.py:13-20), the desert in the middle
FIXED_TERRAIN = ["Mountains", "Pastures", "Forest", "Fields", "Hills", "Pastures", "Hills", "Fields", "Forest", "Desert", "Forest",
                 "Mountains", "Forest", "Mountains", "Fields", "Pastures", "Hills", "Fields", "Pastures"]
# tokens along NUMBER_PLACEMENT_INDS: a 6 on tile 0 and an 8 on tile 3, which touch (tile 9, the desert, is placed last)
RED_PAIR = [6, 8, 5, 2, 3, 10, 9, 12, 11, 4, 8, 10, 9, 4, 5, 6, 3, 11]
LAYOUTS = [
    {"fixed_terrain_placements": FIXED_TERRAIN},
    {"fixed_number_order": RED_PAIR},
    {"fixed_terrain_placements": FIXED_TERRAIN, "fixed_number_order": RED_PAIR},
    {"randomise_number_placement": False},
]


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


_REAL_BOARD = ref_game.Board


def layout_board(layout):
    """a Board whose reset applies `layout` (terrains as the reference's Terrain members, as its own callers would pass them)"""
    randomise, terrain, numbers = spec.normalise_board_config(layout)
    terrain = None if terrain is None else [Terrain(t) for t in terrain]

    class LayoutBoard(_REAL_BOARD):
        def __init__(self, **_ignored):
            _REAL_BOARD.__init__(self, randomise_number_placement=randomise)

        def reset(self):
            self.randomise_number_placement = randomise
            self.fixed_terrain_placements = None if terrain is None else list(terrain)
            self.fixed_number_order = None if numbers is None else list(numbers)
            _REAL_BOARD.reset(self)
    return LayoutBoard


def with_layout(layout, fn):
    ref_game.Board = layout_board(layout)
    try:
        return fn()
    finally:
        ref_game.Board = _REAL_BOARD


def gen_resets():
    out = np.zeros((len(LAYOUTS), len(SEEDS), PAIRS, spec.STATE_WORDS), dtype=np.int32)
    for li, lay in enumerate(LAYOUTS):
        for si, seed in enumerate(SEEDS):
            for p in range(PAIRS):
                def one():
                    e = rh.RefEnv(seed, 100 + PAIRS * li + p)
                    e.reset()
                    return e.state_blob()
                out[li, si, p] = with_layout(lay, one)
    return out


def gen_traj(layout, seed, env_id, steps):
    def run():
        rng = np.random.default_rng(seed * 7919 + env_id)
        e = rh.RefEnv(seed, env_id)
        e.reset()
        acts, crcs, mcrcs, rews, dones = [], [], [], [], []
        for _ in range(steps):
            crcs.append(crc(e.state_blob()))
            mcrcs.append(crc(np.packbits(rh.masks_flat(e.masks()).astype(np.uint8), bitorder="little")))
            a = rh.random_legal_action(e.masks(), e.env, rng)
            _, rew, done = e.step(a)
            acts.append(a); rews.append(rew); dones.append(done)
            if done:
                e.reset()
        return (np.array(acts, dtype=np.int8), np.array(crcs, dtype=np.uint32), np.array(mcrcs, dtype=np.uint32),
                np.array(rews, dtype=np.float32), np.array(dones, dtype=np.uint8), e.state_blob())
    return with_layout(layout, run)


def gen_mt(layout, s, steps):
    def run():
        np.random.seed(s); random.seed(s)
        env = rh.EnvWrapper()
        env.reset()
        arng = np.random.default_rng(1000 + s)
        acts, crcs, dones = [], [], []
        for _ in range(steps):
            crcs.append(crc(rh.state_blob(env, 0)))
            a = rh.random_legal_action(env.get_action_masks(), env, arng)
            _, _, done, _ = env.step(rh.action_to_heads(a))
            acts.append(a); dones.append(done)
            if done:
                env.reset()
        return np.array(acts, dtype=np.int8), np.array(crcs, dtype=np.uint32), np.array(dones, dtype=np.uint8), rh.state_blob(env, 0)
    return with_layout(layout, run)


def main():
    out = {"seeds": np.array(SEEDS, dtype=np.int64), "pairs": PAIRS}
    for li, lay in enumerate(LAYOUTS):
        randomise, terrain, numbers = spec.normalise_board_config(lay)
        out[f"layout{li}_randomise"] = int(randomise)
        out[f"layout{li}_terrain"] = np.array(terrain if terrain is not None else [-1] * 19, dtype=np.int8)
        out[f"layout{li}_numbers"] = np.array(numbers if numbers is not None else [-1] * 18, dtype=np.int8)
    out["reset_blobs"] = gen_resets()
    for k, (li, (seed, env_id)) in enumerate(zip(TRAJ_LAYOUT, TRAJ_SEEDS)):
        a, c, m, r, d, fin = gen_traj(LAYOUTS[li], seed, env_id, TRAJ_STEPS)
        print(f"trajectory {k}: layout {li}, seed {seed}, env {env_id}: {int(d.sum())} game ends in {len(d)} steps")
        assert d.sum() >= 2
        out.update({f"traj{k}_layout": li, f"traj{k}_seed": seed, f"traj{k}_env_id": env_id, f"traj{k}_actions": a,
                    f"traj{k}_state_crc": c, f"traj{k}_mask_crc": m, f"traj{k}_rewards": r, f"traj{k}_dones": d, f"traj{k}_final_blob": fin})
    a, c, d, fin = gen_mt(LAYOUTS[3], MT_SEED, MT_STEPS)
    print(f"mt19937: seed {MT_SEED}: {int(d.sum())} game ends in {len(d)} steps")
    assert d.sum() >= 1
    out.update({"mt_layout": 3, "mt_seed": MT_SEED, "mt_actions": a, "mt_crc": c, "mt_dones": d, "mt_final": fin})
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
