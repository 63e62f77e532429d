"""Pins the CPU oracle against golden vectors captured from the imported upstream reference
(tools/gen_golden.py).  Runs on CPU, needs only /root/repo."""
import numpy as np
import pytest

import golden_util as gu
from settlers_of_catan_rl_amd import spec


def test_topology(oracle):
    g = gu.load("topology.npz")
    t = oracle.topology()
    assert np.array_equal(t["tile_corner"], g["tile_corner"])
    assert np.array_equal(t["tile_edge"], g["tile_edge"])
    assert np.array_equal(t["edge_corner"], g["edge_corner"])
    assert np.array_equal(t["corner_nbr_corner"], g["corner_nbr_corner"])
    assert np.array_equal(t["corner_nbr_edge"], g["corner_nbr_edge"])
    assert np.array_equal(t["corner_tile"], g["corner_tile"])
    assert np.array_equal(t["harbour_slot_corner"], g["harbour_slot_corner"])
    assert np.array_equal(t["harbour_slot_edge"], g["harbour_slot_edge"])
    nbr = t["tile_nbr"]
    assert np.array_equal([sum(1 << v for v in row if v >= 0) for row in nbr], g["tile_nbr_mask"])


def test_device_topology_tables_match_reference():
    """The tables compiled into the HIP kernels (tools/gen_topology.py, geometric derivation)."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(gu.GOLDEN), "..", "tools"))
    import gen_topology
    T = gen_topology.build()
    g = gu.load("topology.npz")
    assert np.array_equal(T["tile_corner"], g["tile_corner"])
    assert np.array_equal(T["tile_edge"], g["tile_edge"])
    assert all(sorted(a) == sorted(b) for a, b in zip(T["edge_corner"], g["edge_corner"].tolist()))
    for c in range(54):
        assert sorted(T["corner_nbr_c"][c]) == sorted(x for x in g["corner_nbr_corner"][c] if x >= 0)
        assert sorted(T["corner_nbr_e"][c]) == sorted(x for x in g["corner_nbr_edge"][c] if x >= 0)
        assert sorted(T["corner_tile"][c]) == sorted(x for x in g["corner_tile"][c] if x >= 0)
    assert np.array_equal(T["tile_nbr_mask"], g["tile_nbr_mask"])
    assert gen_topology.PLACEMENT == g["number_placement"].tolist()
    slots = {}
    for s, (a, b) in enumerate(g["harbour_slot_corner"]):
        slots[int(a)] = s; slots[int(b)] = s
    assert [slots.get(c, 255) for c in range(54)] == T["corner_hslot"]
    # the committed .inc is what the generator emits
    inc = os.path.join(os.path.dirname(gu.GOLDEN), "..", "settlers_of_catan_rl_amd", "csrc", "catan_topology.inc")
    import tempfile
    with tempfile.NamedTemporaryFile("r", suffix=".inc") as f:
        gen_topology.emit(f.name)
        assert open(f.name).read() == open(inc).read()


def test_device_topology_code_against_the_reference_tables(tmp_path):
    """The straight-line bitboard helpers the HIP kernels include (catan_topology.inc: topo_blocked / _touched / _edges_at / _tiles_at,
    branch-free on 32-bit halves since round 5) compiled for the HOST and compared, on random and on sparse inputs, with the same sets
    computed from the reference's topology tables (tests/golden/topology.npz): blocked = occupied corners and their neighbours
    (corner.py:24-39), touched = the end corners of a set of edges, edges_at = the edges at a set of corners (edge.py:23-42),
    tiles_at = the tiles with a corner in the set."""
    import ctypes as C
    import os
    import subprocess
    inc = os.path.join(os.path.dirname(gu.GOLDEN), "..", "settlers_of_catan_rl_amd", "csrc", "catan_topology.inc")
    src = tmp_path / "topo.cpp"
    src.write_text(f"""#include <cstdint>
#define CATAN_TABLE static const
#define CATAN_FN static inline
#define CATAN_TOPOLOGY_CODE
#include "{os.path.abspath(inc)}"
extern "C" void run(const uint64_t* a, const uint64_t* lo, const uint32_t* hi, long n, uint64_t* blocked, uint64_t* touched,
                    uint64_t* elo, uint32_t* ehi, uint32_t* tiles) {{
    for (long i = 0; i < n; i++) {{
        blocked[i] = topo_blocked(a[i]); touched[i] = topo_touched(lo[i], hi[i]);
        topo_edges_at(a[i], elo[i], ehi[i]); tiles[i] = topo_tiles_at(a[i]);
    }}
}}
""")
    so = tmp_path / "libtopo.so"
    subprocess.run(["g++", "-O1", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    lib = C.CDLL(str(so))
    g = gu.load("topology.npz")
    rng = np.random.default_rng(5)
    n = 4000
    keep = rng.integers(1, 6, size=n)                        # sparse to dense sets
    def sets(bits):
        v = rng.integers(0, 1 << 62, size=n, dtype=np.uint64) | (rng.integers(0, 4, size=n, dtype=np.uint64) << np.uint64(62))
        for k in range(5):
            v = np.where(keep > k, v & (rng.integers(0, 1 << 62, size=n, dtype=np.uint64) | (rng.integers(0, 4, size=n, dtype=np.uint64) << np.uint64(62))), v)
        return v & np.uint64((1 << bits) - 1) if bits < 64 else v
    a, lo, hi = sets(54), sets(64), sets(8).astype(np.uint32)
    out = [np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)]
    P = lambda x: x.ctypes.data_as(C.c_void_p)
    lib.run(P(a), P(lo), P(hi), C.c_long(n), *[P(x) for x in out])
    nbr = [[int(x) for x in row if x >= 0] for row in g["corner_nbr_corner"]]
    ec = [[int(x) for x in row] for row in g["edge_corner"]]
    tc = [[int(x) for x in row] for row in g["tile_corner"]]
    for i in range(n):
        occ, roads = int(a[i]), int(lo[i]) | (int(hi[i]) << 64)
        blocked = occ | sum(1 << c for c in range(54) if any((occ >> x) & 1 for x in nbr[c]))
        touched = 0
        for e in range(72):
            if (roads >> e) & 1:
                touched |= (1 << ec[e][0]) | (1 << ec[e][1])
        edges = sum(1 << e for e in range(72) if (occ >> ec[e][0]) & 1 or (occ >> ec[e][1]) & 1)
        tiles = sum(1 << t for t in range(19) if any((occ >> c) & 1 for c in tc[t]))
        assert int(out[0][i]) == blocked and int(out[1][i]) == touched, i
        assert int(out[2][i]) | (int(out[3][i]) << 64) == edges and int(out[4][i]) == tiles, i


def test_reset_states(oracle):
    g = gu.load("reset_states.npz")
    seed = int(g["seed"])
    for env_id, blob in enumerate(g["blobs"]):
        e = oracle.OracleEnv(seed, env_id)
        e.reset()
        ob = e.export()
        assert np.array_equal(ob, blob), spec.describe_state_diff(blob, ob)


def _assert_rule_event(t):
    """The case a rule-case trajectory was recorded for, read off the REFERENCE's own data around `event_step` (its blobs before and
    after the step, its masks, the action): a regenerated fixture that no longer holds its case fails here."""
    f = spec.state_field
    event, s = gu.traj_event(t)
    before, after = gu.traj_sample(t, s), gu.traj_sample(t, s + 1)
    a = t["actions"][s].astype(np.int32)
    m = gu.unpack_masks(t["masks"][s])
    M = spec.MASK_OFFSETS
    actor = int(f(before, "players_go")[0])
    vp = lambda b: np.array([int(f(b, f"p{q}_vp")[0]) for q in (1, 2, 3, 4)])
    if event.startswith("lr_"):
        # a settlement on the title holder's road (game.py:880-912); the builder's own +1 VP is taken out of the VP change
        p, n = int(f(before, "lr_player")[0]), int(f(before, "lr_count")[0])
        q, n2 = int(f(after, "lr_player")[0]), int(f(after, "lr_count")[0])
        assert p != 0 and a[0] == 0 and not f(before, "initial_phase")[0] and actor != p
        dvp = vp(after) - vp(before)
        dvp[actor - 1] -= 1
        paths = [int(x) for x in f(after, "cur_longest_path")]
        mine, others = paths[p - 1], [paths[o - 1] for o in (1, 2, 3, 4) if o != p]
        assert mine < n, "the holder's road was not cut"
        want = [0, 0, 0, 0]
        if event in ("lr_takeover", "lr_takeover_order", "lr_takeover_after_tie"):
            assert q not in (0, p) and n2 == paths[q - 1] == max(others) > mine and n2 >= 5 and others.count(n2) == 1
            if event == "lr_takeover":
                assert sum(x > mine for x in others) == 1
            elif event == "lr_takeover_order":
                assert sum(x > mine for x in others) >= 2
            else:       # in the order of game.py:886 a player level with the holder comes before the new holder: the tie flag is set, then dropped
                order = [o for o in (1, 2, 3, 4) if o != p]
                assert any(paths[o - 1] == mine for o in order[:order.index(q)])
            want[p - 1], want[q - 1] = -2, 2
        elif event == "lr_tie_keep":
            assert q == p and n2 == mine >= 5 and max(others) == mine
        elif event == "lr_tie_vacate":
            assert q == 0 and n2 == 0 and max(others) >= 5 and max(others) > mine and others.count(max(others)) >= 2
            want[p - 1] = -2
        else:
            assert event == "lr_none_vacate" and q == 0 and n2 == 0 and max(others + [mine]) < 5
            want[p - 1] = -2
        assert dvp.tolist() == want, (event, dvp.tolist())
        if q == 0:      # somebody claims the vacant title again inside the replay, with a road (game.py:874-878)
            c = int(t["claim_step"])
            b0, b1 = gu.traj_sample(t, c), gu.traj_sample(t, c + 1)
            who = int(f(b0, "players_go")[0])
            assert s < c < len(t["actions"]) - 1 and t["actions"][c][0] == 1 and int(f(b0, "lr_player")[0]) == 0
            assert int(f(b1, "lr_player")[0]) == who and int(f(b1, "lr_count")[0]) == int(f(b1, "cur_longest_path")[who - 1]) >= 5
            assert (vp(b1) - vp(b0)).tolist() == [2 * (o == who) for o in (1, 2, 3, 4)]
    elif event == "rb_dummy_edge":
        # road building with no legal edge: only the dummy edge 72 is offered, and taking it places nothing
        assert f(before, "road_building_active")[0] == 1 and m[:13].tolist() == [0, 1] + [0] * 11
        assert np.flatnonzero(m[M[2]:M[2] + 73]).tolist() == [72] and a[0] == 1 and a[2] == 72
        assert np.array_equal(f(before, "edge_owner"), f(after, "edge_owner"))
        cnt = int(f(before, "road_building_count")[0])
        assert (int(f(after, "road_building_active")[0]), int(f(after, "road_building_count")[0])) == ((1, 1) if cnt == 0 else (0, 0))
    elif event == "yop_bank_short":
        # Year of Plenty offered while the bank lacks a resource: that resource's bit is 0 in both resource heads
        # (wrapper.py:267-269), and a pick of it (accepted by validate_action only) is skipped (game.py:684-689)
        bank = f(before, "bank_res")
        r1, r2 = int(a[15]), int(a[16])
        assert a[0] == 4 and a[4] == 2 and m[4] == 1 and m[M[4] + 2] == 1
        assert bank[r1] == 0 and bank[r2] > 0 and m[M[10] + r1] == 0 and m[M[9] + 10 + r1] == 0 and m[M[10] + r2] == 1
        assert np.array_equal(m[M[10]:M[10] + 5], (bank > 0).astype(np.float32))
        d_bank, d_res = f(after, "bank_res") - bank, f(after, f"p{actor}_res") - f(before, f"p{actor}_res")
        want = np.zeros(5, dtype=np.int32); want[r2] = 1
        assert np.array_equal(d_res, want) and np.array_equal(d_bank, -want)
        assert f(after, f"p{actor}_n_played")[0] == f(before, f"p{actor}_n_played")[0] + 1
    else:
        # wheat >= 2, ore >= 3 and a settlement to upgrade, but no city piece left: no city offered (wrapper.py:245-250)
        assert event == "city_none_left"
        res = f(before, f"p{actor}_res")
        assert m[10] == 1 and res[4] >= 2 and res[2] >= 3 and f(before, "cities_left")[actor - 1] == 0
        assert ((f(before, "corner_bld") == 1) & (f(before, "corner_owner") == actor)).any()
        assert m[2] == 0 and a[0] != 2


@pytest.mark.parametrize("name", gu.TRAJS + gu.RULE_TRAJS)
def test_trajectory(oracle, name):
    t = gu.load(name)
    e = oracle.OracleEnv(int(t["seed"]), int(t["env_id"]))
    dense, anneal, trades, max_actions = gu.traj_kwargs(t)
    e.set_config(max_trades_per_turn=trades, dense_reward=dense, reward_annealing_factor=anneal, max_actions_per_turn=max_actions)
    e.reset()
    sample = {int(i): k for k, i in enumerate(t["sample_idx"])}
    obs_gold = gu.decode_obs(t)
    n = len(t["actions"])
    for step in range(n):
        blob = e.export()
        assert gu.crc(blob) == int(t["state_crc"][step]), f"state crc differs at step {step}"
        assert np.array_equal(e.masks(), gu.unpack_masks(t["masks"][step])), f"masks differ at step {step}"
        assert e.deciding_player() == int(t["deciding"][step])
        if step in sample:
            k = sample[step]
            assert np.array_equal(blob, t["sample_blob"][k].astype(np.int32)), spec.describe_state_diff(t["sample_blob"][k].astype(np.int32), blob)
            f, lists, lens, pid = e.obs()
            assert np.array_equal(f, obs_gold[k]), f"obs differs at step {step}: {np.flatnonzero(f != obs_gold[k])[:8]}"
            assert np.array_equal(lists, t["sample_lists"][k]) and np.array_equal(lens, t["sample_lens"][k]) and pid == int(t["sample_pid"][k])
        a = t["actions"][step].astype(np.int32)
        assert e.is_legal(a)
        rew, done = e.step(a)
        assert np.array_equal(rew, t["rewards"][step]) and done == bool(t["dones"][step]), step
        if "rewards64" in t.files:      # the reference's Python-float rewards, before the single rounding to fp32
            assert np.array_equal(e.last_reward64(), t["rewards64"][step]), step
        if done:
            e.reset()
    assert np.array_equal(e.export(), t["final_blob"])
    if name in gu.TRAJS:
        assert t["dones"].sum() >= 1
    else:
        assert name == f"traj_rule_{gu.traj_event(t)[0]}.npz"
        _assert_rule_event(t)


def test_mt19937_known_answer(oracle):
    """Config 1: the oracle in Mersenne-Twister mode against the UNPATCHED reference seeded with
    np.random.seed(s); random.seed(s) - pins the numpy/CPython draw semantics of SURVEY 8.4."""
    g = gu.load("mt_kat.npz")
    for s in g["seeds"]:
        s = int(s)
        e = oracle.OracleEnv(mt_seeds=(s, s))
        e.board_reset(); e.reset(); e.reset()          # Board() + Game() constructors, then EnvWrapper.reset()
        acts, crcs = g[f"actions_{s}"], g[f"crc_{s}"]
        for t in range(len(acts)):
            b = e.export(); b[-1] = 0
            assert gu.crc(b) == int(crcs[t]), (s, t)
            _, done = e.step(acts[t].astype(np.int32))
            if done:
                e.reset()
        b = e.export(); b[-1] = 0
        assert np.array_equal(b, g[f"final_{s}"])


def test_longest_road_cases(oracle):
    g = gu.load("longest_road.npz")
    assert len(g["length"]) > 300
    for eo, co, p, ln in zip(g["edge_owner"], g["corner_owner"], g["player"], g["length"]):
        assert oracle.longest_path_raw(eo.astype(np.int32), co.astype(np.int32), int(p)) == int(ln)


def test_gae_and_ppo_loss(oracle):
    """RL/ppo/process_batch.py:134-142 and RL/ppo/ppo.py:54-66, tolerance 1e-5 (north_star)."""
    g = gu.load("gae_ppo.npz")
    for ci in range(3):
        ret, adv = oracle.gae(g[f"gae{ci}_rewards"], g[f"gae{ci}_values"], g[f"gae{ci}_masks"], 0.999, 0.95)
        assert np.allclose(ret, g[f"gae{ci}_returns"], rtol=1e-5, atol=1e-3)     # returns are O(100..1000)
        assert np.allclose(adv, g[f"gae{ci}_adv"], rtol=1e-4, atol=1e-5)
    for ci in range(2):
        la, lv, dl, dv = oracle.ppo_loss(g[f"ppo{ci}_logp"], g[f"ppo{ci}_old"], g[f"ppo{ci}_adv"], g[f"ppo{ci}_v"],
                                         g[f"ppo{ci}_v_old"], g[f"ppo{ci}_ret"], 0.2, 1.0)
        assert abs(la - float(g[f"ppo{ci}_action_loss"])) < 1e-5
        assert abs(lv - float(g[f"ppo{ci}_value_loss"])) < 1e-5
        assert np.allclose(dl, g[f"ppo{ci}_dlogp"], atol=1e-6)
        assert np.allclose(dv, g[f"ppo{ci}_dv"], atol=1e-6)

    # the reference's own PPO.update (ppo.py:26-79) on one minibatch: gradients seen by hooks on the values / log-probs, the
    # returned losses (value x coef, action); the value normaliser of lines 46-48 is applied here as the reference's class does
    for ci in range(3):
        norm = (lambda x: (x - 150.0) / (150.0 + 1e-4)) if int(g[f"ppoU{ci}_use_norm"]) else (lambda x: x)
        coef = float(g["ppoU_value_loss_coef"])
        la, lv, dl, dv = oracle.ppo_loss(g[f"ppoU{ci}_logp"], g[f"ppoU{ci}_old"], g[f"ppoU{ci}_adv"], g[f"ppoU{ci}_v"],
                                         norm(g[f"ppoU{ci}_v_old"].astype(np.float64)).astype(np.float32),
                                         norm(g[f"ppoU{ci}_ret"].astype(np.float64)).astype(np.float32), float(g["ppoU_clip"]), coef)
        assert abs(la - float(g[f"ppoU{ci}_action_loss"])) < 1e-5
        assert abs(lv * coef - float(g[f"ppoU{ci}_value_loss_x_coef"])) < 1e-5
        assert np.allclose(dl, g[f"ppoU{ci}_dlogp"], atol=1e-7, rtol=1e-4)
        assert np.allclose(dv, g[f"ppoU{ci}_dv"], atol=1e-7, rtol=1e-3)


def test_state_layout_constants(oracle):
    assert spec.STATE_WORDS == oracle.STATE_WORDS == 736
    assert spec.MASK_WORDS == oracle.MASK_WORDS == 325


def test_resource_conservation_property(oracle):
    """bank + hands == 19 per resource at every step of random play (reference game rule)."""
    b = oracle.OracleBatch(64, seed=99)
    for _ in range(40):
        blobs = b.run_random(50)
        bank = spec.state_field(blobs, "bank_res")
        tot = bank.copy()
        for p in (1, 2, 3, 4):
            tot = tot + spec.state_field(blobs, f"p{p}_res")
        assert (tot == 19).all()
        assert (spec.state_field(blobs, "p1_res") >= 0).all()


def test_randomise_uncertainty_golden(oracle):
    """Game.randomise_uncertainty (game.py:1207-1282): states before / after from the reference (tools/gen_golden.py)."""
    g = gu.load("randomise.npz")
    seed = int(g["seed"])
    for before, after, ctrl, env_id in zip(g["before"], g["after"], g["ctrl"], g["env_id"]):
        e = oracle.OracleEnv(seed, int(env_id))
        e.import_(before)
        e.randomise_uncertainty(int(ctrl))
        out = e.export()
        assert np.array_equal(out, after), spec.describe_state_diff(after, out)


def test_validate_cases(oracle):
    """SURVEY a4 - validate mode = `_translate_action` + `Game.validate_action` (game/game.py:264-525), the wrapper's default
    (env/wrapper.py:13,38-41): the reference's own accept / reject on 8 800 probe actions (all 13 types; in-range, out-of-range,
    targeted) in 720 of its states, and - for every accepted probe, incl. the ~500 that NO mask offers (MoveRobber onto an
    empty tile, ProposeTrade past the limit, RollDice during road building, the dummy edge, ...) - its state / masks / rewards /
    done afterwards."""
    g = {k: v for k, v in gu.load("validate_cases.npz").items()}       # (an NpzFile decompresses on every access)
    acc, inm = g["case_accept"].astype(bool), g["case_in_masks"].astype(bool)
    assert len(acc) > 8000 and (acc & ~inm).sum() > 400 and (~acc).sum() > 4000
    blob_at = {int(c): k for k, c in enumerate(g["post_blob_case"])}
    for c in range(len(acc)):
        si = int(g["case_state"][c])
        tr, ma = int(g["state_trades"][si]), int(g["state_max_actions"][si])
        e = oracle.OracleEnv(int(g["state_seed"][si]), int(g["state_env"][si]))
        e.set_config(max_trades_per_turn=None if tr < 0 else tr, max_actions_per_turn=None if ma < 0 else ma)
        e.import_(g["states"][si].astype(np.int32))
        a = g["case_action"][c]
        assert e.is_legal(a) == bool(acc[c]), (c, a.tolist(), bool(acc[c]))
        ai = np.ascontiguousarray(a, dtype=np.int32)
        in_masks = bool(e.L.orc_action_in_masks(e.p, oracle._p(ai, oracle.C.c_int32)))
        if int(a[0]) != 6:
            assert in_masks == bool(inm[c]), (c, a.tolist())
        if not acc[c]:
            continue
        rew, done = e.step(a)
        post = e.export()
        if c in blob_at:
            want = g["post_blobs"][blob_at[c]].astype(np.int32)
            assert np.array_equal(post, want), f"case {c} {a.tolist()}:\n" + spec.describe_state_diff(want, post)
        assert gu.crc(post) == int(g["post_crc"][c]), (c, a.tolist())
        assert np.array_equal(e.masks(), gu.unpack_masks(g["post_masks"][c])), c
        assert np.array_equal(e.last_reward64(), g["post_reward64"][c]) and done == bool(g["post_done"][c]), c
        assert e.deciding_player() == int(g["post_deciding"][c]), c
