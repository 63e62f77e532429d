"""The playout player's decision (catan_playout_actions, include/catan_hip_tuning.h) restated over the CPU oracle: test
infrastructure for the device entry point.  It shares no code with the kernels: every sim slot is an oracle env of its own, seeded with
the sim handle's seed and the slot's global game id, that imports the root's exported blob with the draw counter moved on; the candidates
come from the numpy restatements of the rule-based players (scripted_reference, trader_reference) and the oracle's random sampler; the
hold rule, the integer score, the duplicate rule and the tie rule are written out below.

    decide(root_blobs, games, cfg, sim_seed, sim_env_id0) -> Result(actions [rows,18], chosen [rows], stats [rows,C,7], cand, dup, invalid)

`cfg` is a dict with the fields of catan_playout_cfg_t (builder, trader, randoms, playouts, depth, playout_style 0/1 or a name,
determinise, step_idx).  The keyword `variant` plants an error on purpose (the tests show that their fixtures can tell them apart):
"tie_high" (ties to the highest index), "no_latch" (a finished slot is held for one step only), "min_opponent" (the margin against the
weakest opponent)."""
from collections import namedtuple

import numpy as np

import oracle_lib
import scripted_reference as sr
import trader_reference as tr
from settlers_of_catan_rl_amd import spec

Result = namedtuple("Result", "actions chosen stats cand dup invalid")
FIELDS = {name: i for i, name in enumerate(spec.PLAYOUT_STAT_FIELDS)}
STYLES = {"builder": 0, "trader": 1, 0: 0, 1: 1}
ENDTURN_ROW = np.array([sr.ENDTURN] + [0] * 17, dtype=np.int32)
_RNG = spec.STATE_OFFSETS["rng_draws"][0]


def deciding_player(blob):
    """PlayerId 1..4 of the player who decides in this state"""
    return sr.deciding_pid0(blob) + 1


def scripted_action(style, blob, masks):
    return (tr.decide(blob, masks) if STYLES[style] == 1 else sr.decide(blob, masks))[0]


def playout_score(blob, p, variant=None):
    """(finished, won, score, vp of p) of one final position for PlayerId p"""
    winner = int(spec.state_field(blob, "winner")[0])
    vp = [int(spec.state_field(blob, f"p{q}_vp")[0]) for q in (1, 2, 3, 4)]
    others = [vp[q] for q in range(4) if q != p - 1]
    margin = vp[p - 1] - (min(others) if variant == "min_opponent" else max(others))
    won = int(winner == p)
    return int(winner != 0), won, spec.PLAYOUT_WIN_SCORE * won + spec.PLAYOUT_VP_SCORE * margin, vp[p - 1]


def pick(valid, score_sums, variant=None):
    """the valid candidate with the largest score sum; ties to the lowest index"""
    best = None
    for c, (v, s) in enumerate(zip(valid, score_sums)):
        if not v:
            continue
        if best is None or s > score_sums[best] or (variant == "tie_high" and s == score_sums[best]):
            best = c
    return best


def mark_duplicates(cand):
    """cand [C,18] -> bool [C]: bytewise equal to a lower-numbered candidate"""
    return np.array([any((cand[c] == cand[o]).all() for o in range(c)) for c in range(len(cand))], dtype=bool)


def _slot_env(blob, sim_seed, sim_env_id0, slot, k, limits):
    env = oracle_lib.OracleEnv(sim_seed, sim_env_id0 + slot)
    env.set_config(max_trades_per_turn=limits[0], max_actions_per_turn=limits[1])
    b = np.array(blob, dtype=np.int32)
    b[_RNG] = np.uint32((int(np.uint32(b[_RNG])) + ((1 + k) << spec.PLAYOUT_DRAW_SHIFT)) & 0xFFFFFFFF).astype(np.int32)
    env.import_(b)
    return env


def decide(root_blobs, games, cfg, sim_seed, sim_env_id0, limits=(4, None), variant=None):
    root_blobs = np.asarray(root_blobs, dtype=np.int32)
    n_root = root_blobs.shape[0]
    games = list(range(n_root)) if games is None else [int(g) for g in games]
    nb, nt, nr = int(cfg["builder"]), int(cfg["trader"]), int(cfg["randoms"])
    C, K, depth = nb + nt + nr, int(cfg["playouts"]), int(cfg["depth"])
    style, determinise, step_idx = STYLES[cfg["playout_style"]], bool(cfg["determinise"]), int(cfg["step_idx"])
    rows = len(games)
    actions = np.zeros((rows, 18), dtype=np.int32)
    chosen = np.zeros(rows, dtype=np.int32)
    stats = np.zeros((rows, C, spec.PLAYOUT_STAT_WORDS), dtype=np.int64)
    cands = np.zeros((rows, C, 18), dtype=np.int32)
    dups = np.ones((rows, C), dtype=bool)
    invalid = 0
    for j, g in enumerate(games):
        if g < 0 or g >= n_root:
            actions[j], chosen[j] = ENDTURN_ROW, -1
            continue
        blob = root_blobs[g]
        p = deciding_player(blob)
        slot = lambda c, k: (j * C + c) * K + k
        # the candidates: sampled in the slots (j, c, 0), before anything is re-dealt
        for c in range(C):
            env = _slot_env(blob, sim_seed, sim_env_id0, slot(c, 0), 0, limits)
            b0, m0 = env.export(), env.masks()
            if c < nb:
                cands[j, c] = sr.decide(b0, m0)[0]
            elif c < nb + nt:
                cands[j, c] = tr.decide(b0, m0)[0]
            else:
                cands[j, c] = env.sample_action(sim_seed, sim_env_id0 + slot(c, 0), step_idx, m0)
        dups[j] = mark_duplicates(cands[j])
        sums = []
        for c in range(C):
            if dups[j, c]:
                sums.append(0)
                continue
            row = stats[j, c]
            row[FIELDS["valid"]], row[FIELDS["sims"]] = 1, K
            for k in range(K):
                env = _slot_env(blob, sim_seed, sim_env_id0, slot(c, k), k, limits)
                if determinise:
                    env.randomise_uncertainty(p)
                held, done_prev, steps = False, False, 0
                for d in range(depth):
                    if d == 0:
                        a = cands[j, c]
                    else:
                        held = done_prev if variant == "no_latch" else (held or done_prev)
                        if held:
                            done_prev = False             # a no-op reports done = 0
                            continue
                        a = scripted_action(style, env.export(), env.masks())
                    steps += 1
                    if not env.is_legal(a):               # the device leaves the game alone and counts the action
                        invalid += 1
                        done_prev = False
                        continue
                    _, done_prev = env.step(a)
                fin, won, score, vp = playout_score(env.export(), p, variant)
                row[FIELDS["finished"]] += fin; row[FIELDS["wins"]] += won; row[FIELDS["score_sum"]] += score
                row[FIELDS["vp_sum"]] += vp; row[FIELDS["steps_sum"]] += steps
            sums.append(int(row[FIELDS["score_sum"]]))
        best = pick(~dups[j], sums, variant)
        actions[j], chosen[j] = cands[j, best], best
    return Result(actions, chosen, stats, cands, dups, invalid)


# ---------------------------------------------------------------------------------------------- the shared fixture
# 16 oracle games of seed FIXTURE_SEED, game i advanced by FIXTURE_COUNTS[i] uniform-random decisions: initial placements, normal turns,
# answers to offers and a discard are among the roots (tests/test_playout_reference_cpu.py asserts it).
FIXTURE_SEED, FIXTURE_COUNTS = 1, [2, 5, 9, 13, 30, 60, 90, 120, 150, 200, 260, 330, 410, 500, 600, 700]
SIM_SEED, SIM_ENV_ID0 = 5, 1 << 40
_fixture = None


def fixture_roots():
    """-> int32 [16, 736] (a copy)"""
    global _fixture
    if _fixture is None:
        _fixture = oracle_lib.OracleBatch(len(FIXTURE_COUNTS), FIXTURE_SEED, 0).run_random_counts(FIXTURE_COUNTS)
    return _fixture.copy()


def root_phases(blobs):
    """-> per root one of "discard", "respond", "initial", "turn", "over" """
    out = []
    for b in np.asarray(blobs):
        f = lambda name: int(spec.state_field(b, name)[0])
        out.append("over" if f("winner") else "discard" if f("n_to_discard") > 0 else "respond" if f("must_respond") else "initial" if f("initial_phase") else "turn")
    return out


def near_win_root():
    """A planted position: player 1, to move after the roll, owns a settlement on corner 0, stands at 9 victory points and holds exactly
    a city's price (three ore, two wheat, taken from the bank).  Upgrading that settlement wins the game at once."""
    env = oracle_lib.OracleEnv(1, 0)
    env.reset()
    b = env.export().copy()
    put = lambda name, v: spec.state_field(b, name).__setitem__(slice(None), v)
    for name in ("corner_bld", "corner_owner", "edge_owner"):
        put(name, 0)
    for p in (1, 2, 3, 4):
        put(f"p{p}_res", 0); put(f"p{p}_vis", 0); put(f"p{p}_harbours", 0); put(f"p{p}_vp", 2)
    put("bank_res", [19, 19, 16, 19, 17])
    put("p1_res", [0, 0, 3, 0, 2])
    put("settlements_left", [4, 5, 5, 5]); put("cities_left", 4)
    spec.state_field(b, "corner_bld")[0] = 1
    spec.state_field(b, "corner_owner")[0] = 1
    put("player_order", [1, 2, 3, 4]); put("player_order_id", 0); put("players_go", 1)
    put("initial_phase", 0); put("init_settlements", 2); put("init_roads", 2)
    put("dice_rolled", 1)
    put("curr_vps", [9, 2, 2, 2]); put("p1_vp", 9)
    return b
