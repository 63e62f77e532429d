"""GPU: the start pool's weighted pick and per-entry outcome tallies (csrc/catan_hooks.hip) - 64 games, the
scenario of tests/test_gpu_start_pool.py (both 32-game tiles of k_step, a global id base whose words are both non-zero, the rule-based
player in every seat).  The twin is tests/start_pool_weighted_reference.py: the CPU oracle with the weighted rule applied by export /
import and the outcome table kept in Python integers.  Every comparison is integer (or bit) equality.  Weights, seeds and caps come from
the reference module and are checked on the CPU by tests/test_start_pool_weighted_cpu.py::test_seed_check_for_the_gpu_scenarios."""
import ctypes as C

import numpy as np
import pytest
import torch

import episode_stats_oracle as eso
import league_stats_oracle as lso
import record_reference as rr
import start_pool_reference as spr
import start_pool_weighted_reference as wr
from settlers_of_catan_rl_amd import spec

pytestmark = pytest.mark.gpu

N, SEED, ID0 = wr.N_GAMES, wr.SEED, wr.ENV_ID0
EINVAL = -1


@pytest.fixture(scope="module")
def pools():
    p = wr.pools()
    for v in p.values():
        v.setflags(write=False)
    return p


def _env(env_id0=ID0, auto_reset=True, n=N, **kw):
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    return VecCatanEnv(n, seed=SEED, env_id0=env_id0, auto_reset=auto_reset, **kw)


def _pair(pool, fresh_q16=0, weights=None, focus=wr.FOCUS, outcomes=True):
    """an env and its twin under the same pool, weights and outcome settings; nothing dealt yet"""
    env, twin = _env(), wr.OutcomeTwin(N, SEED, ID0, pool, fresh_q16, weights)
    env.set_start_pool(pool, fresh_share=fresh_q16 / 65536.0, weights=weights)
    if outcomes:
        env.enable_start_pool_outcomes(None if focus is None else torch.from_numpy(np.asarray(focus)))
        twin.enable_outcomes(focus)
    return env, twin


def _same_state(env, twin, where):
    got, want = env.export_state().cpu().numpy(), twin.blobs()
    for g in range(env.n):
        assert np.array_equal(got[g], want[g]), (where, g, spec.describe_state_diff(got[g], want[g]))
    assert np.array_equal(env.get_action_masks().cpu().numpy(), twin.masks()), where


def _same_counts(env, twin):
    c, w = env.start_pool_counts(), twin.counts
    assert (c["pool"], c["fresh"]) == (w["pool"], w["fresh"]) and np.array_equal(c["per_entry"], w["per_entry"]), (c, w)
    return c


def _same_outcomes(env, twin, where=""):
    got, m = env.start_pool_outcomes(), len(twin.pool)
    want = twin.table[2:].reshape(m + 1, wr.ROW)
    assert (got["seen"], got["skipped"]) == (int(twin.table[0]), int(twin.table[1])), (where, got["seen"], got["skipped"], twin.table[:2])
    assert np.array_equal(got["table"], want), (where, np.argwhere(got["table"] != want)[:8])
    return got


def _lockstep(env, twin, steps, every_step=True):
    """reset() under the pool, then `steps` steps with the device's scripted sampler; after every step all blobs, mask rows, rewards, done
    flags, the install counters and the outcome table equal the twin's, which is fed the same action rows"""
    env.reset(); twin.reset()
    _same_state(env, twin, "after reset")
    for t in range(steps):
        a = env.sample_scripted_actions()
        a_h = a.cpu().numpy()
        reward, done = env.step(a)
        r_h, d_h = reward.cpu().numpy().copy(), done.cpu().numpy().copy()
        tr, td = twin.step(torch.from_numpy(a_h))
        assert np.array_equal(r_h, tr.numpy()) and np.array_equal(d_h, td.numpy()), t
        _same_state(env, twin, f"after step {t}")
        if every_step:
            _same_counts(env, twin)
            if twin.table is not None:
                _same_outcomes(env, twin, f"after step {t}")
    assert env.invalid_action_count() == 0 and env.missed_speculation_count() == 0


@pytest.mark.parametrize("fresh_q16", [0, wr.HALF_FRESH_Q16])
def test_weighted_lockstep_equals_the_twin(hip_lib, pools, fresh_q16):
    """weighted parity: the 64-entry pool with zeros, tiny weights and one weight of 2^31, every deal from the pool and half of them"""
    w = wr.weights_64()
    env, twin = _pair(pools[64], fresh_q16, w)
    _lockstep(env, twin, wr.STEP_CAP)
    c, o = _same_counts(env, twin), _same_outcomes(env, twin)
    print("fresh_q16", fresh_q16, "deals", c["pool"], c["fresh"], "finished", o["seen"], "entries tallied", int((o["games"] > 0).sum()), "fresh row", o["fresh"])
    assert all(c["per_entry"][k] == 0 for k in wr.ZEROS_64) and c["per_entry"][wr.HEAVY] >= 8
    assert o["skipped"] == 0 and o["seen"] == len(twin.finished) >= 32 and (o["games"] > 0).sum() >= 8
    assert (o["fresh"]["games"] >= 1) == (fresh_q16 > 0) and (c["fresh"] > 0) == (fresh_q16 > 0)
    # the derived arrays: NaN exactly where nothing was tallied
    assert np.array_equal(np.isnan(o["focus_win_share"]), o["focus_games"] == 0) and np.array_equal(np.isnan(o["win_share_by_pid"][:, 0]), o["games"] == 0)
    played = o["games"] > 0
    assert np.allclose(o["win_share_by_pid"][played].sum(axis=1), 1.0)
    # a read with reset zeroes the table
    assert env.start_pool_outcomes(reset=True)["seen"] == o["seen"] and env.start_pool_outcomes()["seen"] == 0 and not env.start_pool_outcomes()["table"].any()


def _deferred(env, twin, calls, window):
    """tests/test_gpu_start_pool.py's driver: step_deferred with the bot, then the flush; the twin gets exactly the applied rows"""
    waiting, outstanding = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
    want_r, want_d = np.zeros((N, 4), dtype=np.float32), np.zeros(N, dtype=np.uint8)

    def deliver(r_h, d_h, sel):
        assert np.array_equal(r_h[sel], want_r[sel]) and np.array_equal(d_h[sel], want_d[sel])

    for t in range(calls):
        a = env.sample_scripted_actions()
        a_h = a.cpu().numpy().copy()
        applied = ~waiting & (a_h[:, 0] >= 0)
        assert not (applied & outstanding).any()
        a_h[~applied, 0] = -1
        tr, td = twin.step(torch.from_numpy(a_h))
        want_r[applied], want_d[applied] = tr.numpy()[applied], td.numpy()[applied]
        outstanding |= applied
        reward, done, status = env.step_deferred(a, window=window)
        r_h, d_h, s_h = reward.cpu().numpy(), done.cpu().numpy(), status.cpu().numpy()
        got = (s_h == 0) & outstanding
        deliver(r_h, d_h, got)
        outstanding &= ~got
        waiting = s_h == 1
    reward, done, status = env.step_flush()
    r_h, d_h, s_h = reward.cpu().numpy(), done.cpu().numpy(), status.cpu().numpy()
    assert ((s_h == 0) == waiting).all()
    deliver(r_h, d_h, waiting & outstanding)


@pytest.mark.parametrize("window", [1, 4])
def test_deferred_equals_the_twin(hip_lib, pools, window):
    """catan_step_deferred, compared at the flush: states, masks, install counters and the outcome table - the picks and the tallies are those
    of a lock-step run with the same per-game step counts"""
    env, twin = _pair(pools[64], 0, wr.weights_64())
    env.reset(); twin.reset()
    _deferred(env, twin, wr.STEP_CAP, window)
    _same_state(env, twin, "after the flush")
    c, o = _same_counts(env, twin), _same_outcomes(env, twin)
    print("window", window, "deals", c["pool"], "finished", o["seen"])
    assert c["pool"] > 64 + 16 and o["seen"] >= 16 and o["skipped"] == 0 and env.invalid_action_count() == 0


def test_random_rollout_equals_the_twin(hip_lib, oracle, pools):
    """catan_random_rollout (lock-step, the library's uniform-random policy)"""
    env, twin = _pair(pools[64], 0, wr.weights_64())
    env.reset(); twin.reset()
    env.random_rollout(0, spr.RANDOM_STEPS)
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    for s in range(spr.RANDOM_STEPS):
        masks, a = twin.masks(), np.zeros((N, 18), dtype=np.int32)
        for g in range(N):
            twin.L.orc_sample_action(twin.b.env_ptr(g), SEED, ID0 + g, s, masks[g].ctypes.data_as(f32p), a[g].ctypes.data_as(i32p))
        twin.step(torch.from_numpy(a))
    _same_state(env, twin, "after the rollout")
    c, o = _same_counts(env, twin), _same_outcomes(env, twin)
    assert c["pool"] > 64 and o["seen"] == c["pool"] - 64 and o["skipped"] == 0, (c, o["seen"])


def test_reset_with_a_mask_and_without(hip_lib, pools):
    """catan_reset: the selected games take a weighted pick (and its origin), the others keep their state and their origin"""
    w = wr.weights_64()
    env, twin = _pair(pools[64], 0, w)
    sel = np.zeros(N, dtype=bool)
    sel[[0, 5, 31, 32, 63]] = True
    env.reset(torch.from_numpy(sel)); twin.reset(sel)
    _same_state(env, twin, "after the masked reset")
    c = _same_counts(env, twin)
    assert c["pool"] == 5 and all(c["per_entry"][k] == 0 for k in wr.ZEROS_64)
    env.reset(); twin.reset()
    _same_state(env, twin, "after the full reset")
    assert _same_counts(env, twin)["pool"] == 5 + N
    # the origins the resets left are what the tallies of the next games use
    for t in range(60):
        a = env.sample_scripted_actions()
        a_h = a.cpu().numpy()
        env.step(a); twin.step(torch.from_numpy(a_h))
    _same_state(env, twin, "60 steps on")
    assert _same_outcomes(env, twin)["seen"] >= 8


def test_all_ones_weights_give_the_uniform_trajectory(hip_lib, pools):
    """a second handle under the same pool without weights: identical blobs, masks, rewards, done flags and counters at every step"""
    a, b = _env(), _env()
    a.set_start_pool(pools[64], weights=np.ones(64, dtype=np.int64))
    b.set_start_pool(pools[64])
    a.reset(); b.reset()
    dones = 0
    for t in range(150):
        ra, da = a.step(a.sample_scripted_actions())
        rb, db = b.step(b.sample_scripted_actions())
        assert torch.equal(ra, rb) and torch.equal(da, db), t
        assert torch.equal(a.export_state(), b.export_state()) and torch.equal(a.get_action_masks(), b.get_action_masks()), t
        dones += int(da.sum())
    ca, cb = a.start_pool_counts(), b.start_pool_counts()
    assert dones >= 32 and ca["pool"] == cb["pool"] == N + dones and np.array_equal(ca["per_entry"], cb["per_entry"])


def test_weight_on_the_last_entry_alone(hip_lib, pools):
    env, twin = _pair(pools[64], 0, [0] * 63 + [1], outcomes=False)
    _lockstep(env, twin, 40)
    env.reset(); twin.reset()                    # (entry 63 is an early position: no game of it ends within a few steps, so deal them all again)
    _same_state(env, twin, "after the second reset")
    c = _same_counts(env, twin)
    assert c["pool"] == 2 * N and c["per_entry"][63] == c["pool"] and not c["per_entry"][:63].any()
    last = spr._zero_rng(pools[64][63])
    assert sum(spr._zero_rng(b) == last for _g, b in twin.deal_log) == c["pool"]


def test_a_65536_entry_table(hip_lib, pools):
    """the 64 positions tiled to 65 536 entries with weight on entries 0, 63, 64, 4 095, 4 096 and 65 535 alone - the edges of every round of a
    64-ary search: every install hits one of them, with the counts the reference predicts"""
    big = np.tile(pools[64], (wr.BIG_M // 64, 1))
    w = wr.big_weights()
    env, twin = _env(), wr.OutcomeTwin(N, SEED, ID0, big, 0, w.tolist())
    env.set_start_pool(torch.from_numpy(big), weights=torch.from_numpy(w))
    _lockstep(env, twin, 40, every_step=False)
    c = _same_counts(env, twin)
    hit = np.flatnonzero(c["per_entry"])
    print("installs", c["pool"], "entries hit", hit.tolist(), c["per_entry"][hit].tolist())
    assert c["pool"] > N and set(hit.tolist()) <= set(wr.BIG_EDGES) and len(hit) >= 4


def test_set_weights_none_restores_the_uniform_rule(hip_lib, pools):
    env, twin = _pair(pools[64], 0, wr.weights_64(), outcomes=False)
    _lockstep(env, twin, 30)
    env.set_start_pool_weights(None); twin.set_weights(None)
    for t in range(60):
        a = env.sample_scripted_actions()
        a_h = a.cpu().numpy()
        env.step(a); twin.step(torch.from_numpy(a_h))
        _same_state(env, twin, f"uniform again, step {t}")
    c = _same_counts(env, twin)
    assert any(c["per_entry"][k] > 0 for k in wr.ZEROS_64), c["per_entry"]         # the uniform rule installs what the weights kept out
    env.set_start_pool_weights(None)                                                 # without weights: nothing to do


def test_state_handling(hip_lib, pools):
    """weights set twice and over a pool in use; catan_state_import and catan_state_fork clear the origin of the games they overwrite;
    set_start_pool keeps the outcomes on with a zeroed table of the new size, drops the weights and resets the origins, so that the games
    in flight are tallied as fresh ones and not to the new pool's entries"""
    def steps(k, where):
        for t in range(k):
            a = env.sample_scripted_actions()
            a_h = a.cpu().numpy()
            env.step(a); twin.step(torch.from_numpy(a_h))
        _same_state(env, twin, where)
        _same_counts(env, twin)
        return _same_outcomes(env, twin, where)

    env, twin = _pair(pools[64], 0, [1] * 32 + [0] * 32)
    w = wr.weights_64()
    env.set_start_pool_weights(w); twin.set_weights(w)                              # twice: the second table is the one in force
    _lockstep(env, twin, 12)
    w2 = [0] * 32 + [5] * 32
    env.set_start_pool_weights(torch.tensor(w2)); twin.set_weights(w2)              # over a pool in use
    steps(12, "under the second weights")
    assert not (twin.origin < 0).any()
    # import: the same states, so only the origins change; fork: from a second handle that holds this one's states
    blobs = env.export_state()
    env.import_state(blobs[[3, 40]], [3, 40])
    twin.origin[[3, 40]] = -1
    other = _env()
    other.import_state(blobs)
    env.fork_from(other, [5, 6, 63], [5, 6, 63])
    twin.origin[[5, 6, 63]] = -1
    before = int(twin.table[2 + 64 * 8])
    assert before == 0
    o = steps(120, "after import and fork")
    print("fresh row after import / fork", o["fresh"])
    assert o["fresh"]["games"] >= 1 and o["fresh"]["games"] <= 5 and o["seen"] >= 32
    # a new pool
    in_flight = int((twin.origin >= 0).sum())
    env.set_start_pool(pools[3]); twin.set_pool(pools[3])
    assert in_flight > 0 and twin.cum is None and twin.table.shape == (2 + 4 * 8,) and not twin.table.any()
    got = env.start_pool_outcomes()
    assert got["table"].shape == (4, 8) and not got["table"].any() and got["seen"] == 0
    o = steps(150, "under the new pool")
    print("under the new pool: fresh row", o["fresh"], "entries", o["games"].tolist())
    assert o["fresh"]["games"] >= 8 and o["games"].sum() >= 8 and (_same_counts(env, twin)["per_entry"] > 0).all()
    # clear switches the outcomes off with the pool
    from settlers_of_catan_rl_amd._lib import CatanHipError
    env.clear_start_pool()
    with pytest.raises(CatanHipError):
        env.start_pool_outcomes()


def _episodes(finished):
    """the twin's finished games as rows of episode_stats_oracle.replay (DECISION 0: inside every counter)"""
    rows = []
    for g, blob, _origin in finished:
        f = lambda name: spec.state_field(blob, name)
        rows.append([g, 0, int(f("winner")[0]), int(f("turn")[0]), int(f("lr_player")[0]), int(f("la_player")[0])]
                    + [int(f(f"p{p}_vp")[0]) for p in (1, 2, 3, 4)] + [int(x) for x in f("player_order")]
                    + [int(x) for x in f("settlements_left")] + [int(x) for x in f("cities_left")]
                    + [int(f(f"p{p}_n_played")[0]) for p in (1, 2, 3, 4)])
    return np.array(rows, dtype=np.int64).reshape(-1, eso.COLS)


@pytest.mark.parametrize("window", [None, 1, 4], ids=["lockstep", "deferred-1", "deferred-4"])
def test_outcomes_beside_the_other_hooks(hip_lib, pools, window):
    """the finished-game statistics, the league scoreboard and the recorder run at the same hook: each table equals its own oracle over
    the twin's finished games, the outcome table equals the twin's, and the sealed records replay to their final blobs.  Lock-step steps
    reach the re-deal of step_impl and the two installs of the slow path; step_deferred (windows 1 and 4, wr.STEP_CAP calls and the flush,
    every hook on as well: none is refused inside an open sequence, only enabling and reading are) reaches the slow path's two fresh deals,
    on the side stream and on the window's own.  The finished-game bound of the deferred cases is test_deferred_equals_the_twin's (same
    pool, seed and calls); how many records seal there depends on which games wait, so one is asked for and the count is printed."""
    num_nets = 3
    env, twin = _pair(pools[64], 0, wr.weights_64())
    slot, net = lso.maps(N, num_nets, 4)
    env.enable_episode_stats(torch.from_numpy(wr.FOCUS))
    env.enable_league_stats(torch.from_numpy(slot), torch.from_numpy(net), num_nets)
    env.reset(); twin.reset()
    env.enable_recording(list(range(N)), capacity=wr.STEP_CAP)
    env.arm_recording(at_deal=True)
    if window is None:
        for t in range(150):
            a = env.sample_scripted_actions()
            a_h = a.cpu().numpy()
            env.step(a); twin.step(torch.from_numpy(a_h))
        where, min_seen, min_recs = "after 150 steps", 32, 8
    else:
        _deferred(env, twin, wr.STEP_CAP, window)
        where, min_seen, min_recs = "after the flush", 16, 1
    _same_state(env, twin, where)
    o = _same_outcomes(env, twin)
    ep = _episodes(twin.finished)
    assert len(ep) == o["seen"] >= min_seen and o["skipped"] == 0
    want = eso.counters(ep, 0, wr.FOCUS)
    got = env.episode_stats_words()
    assert got == want, (eso.named(got), eso.named(want))
    assert np.array_equal(env.league_stats().numpy(), lso.table(ep, 0, slot, net, num_nets))
    named = spec.episode_stats_dict(got)
    assert named["episodes"] == o["games"].sum() and named["focus_episodes"] == o["focus_games"].sum() and named["focus_wins"] == o["focus_wins"].sum()
    assert named["turns_sum"] == o["turns_sum"].sum()                               # the same field: the final turn number
    recs = env.recordings()
    print("driver", "lock-step" if window is None else f"deferred, window {window}", "finished", o["seen"], "sealed records", len(recs))
    assert len(recs) >= min_recs and env.invalid_action_count() == 0
    for rec in recs[:8]:
        final, _rew, done, rejected = rr.replay_on_cpu(rec.seed, rec.game_id, rec.start_blob, rec.actions, **rec.cfg)
        assert np.array_equal(final, rec.final_blob) and done[-1] and not rejected.any()


def test_error_returns(hip_lib, pools):
    """every CATAN_EINVAL of the three entry points; what was in force before stays as it was"""
    from settlers_of_catan_rl_amd.env import VecCatanEnv, _ptr, _stream
    L = hip_lib
    dev = torch.device("cuda")
    w = wr.weights_64()
    env, twin = _pair(pools[64], 0, w)
    u32 = lambda vals: torch.from_numpy(np.array(vals, dtype=np.uint32).view(np.int32)).to(dev)
    out = np.zeros(2 + 65 * 8, dtype=np.uint64)
    op = out.ctypes.data_as(C.POINTER(C.c_uint64))

    def refused(rc, word):
        assert rc == EINVAL and word.encode() in L.catan_last_error(), (rc, L.catan_last_error())

    good = u32([1] * 64)
    refused(L.catan_start_pool_set_weights(None, _ptr(good), _stream()), "null handle")
    refused(L.catan_start_pool_set_weights(env.h, _ptr(u32([0] * 64)), _stream()), "sum to 0")
    refused(L.catan_start_pool_set_weights(env.h, _ptr(u32([2 ** 31, 2 ** 31] + [0] * 62)), _stream()), "sum to 4294967296")
    refused(L.catan_start_pool_set_weights(env.h, _ptr(u32([2 ** 32 - 1] * 64)), _stream()), "sum to 274877906880")
    refused(L.catan_start_pool_outcomes_enable(None, 1, None, _stream()), "null handle")
    refused(L.catan_start_pool_outcomes_read(env.h, None, 0, _stream()), "null argument")
    assert L.catan_start_pool_outcomes_words() == 8
    # no pool: all three
    bare = _env()
    refused(L.catan_start_pool_set_weights(bare.h, _ptr(good), _stream()), "no start pool")
    refused(L.catan_start_pool_set_weights(bare.h, None, _stream()), "no start pool")
    refused(L.catan_start_pool_outcomes_enable(bare.h, 1, None, _stream()), "no start pool")
    refused(L.catan_start_pool_outcomes_read(bare.h, op, 0, _stream()), "no start pool")
    # a pool, outcomes off
    bare.set_start_pool(pools[3])
    refused(L.catan_start_pool_outcomes_read(bare.h, op, 0, _stream()), "outcomes are not enabled")
    bare.enable_start_pool_outcomes()
    bare.enable_start_pool_outcomes(on=False)
    refused(L.catan_start_pool_outcomes_read(bare.h, op, 0, _stream()), "outcomes are not enabled")
    # a handle that never re-deals
    fixed = _env(auto_reset=False)
    fixed.set_start_pool(pools[3])
    refused(L.catan_start_pool_outcomes_enable(fixed.h, 1, None, _stream()), "auto_reset = 0")
    # a handle under the MT19937 contract
    one = VecCatanEnv(1, seed=3, auto_reset=False)
    one.seed_mt19937(1, 2)
    refused(L.catan_start_pool_set_weights(one.h, _ptr(good), _stream()), "MT19937")
    refused(L.catan_start_pool_outcomes_enable(one.h, 1, None, _stream()), "MT19937")
    # an open deferred sequence
    env.reset(); twin.reset()
    env.step_deferred(env.sample_scripted_actions(), window=4)
    refused(L.catan_start_pool_set_weights(env.h, _ptr(good), _stream()), "deferred step sequence is open")
    refused(L.catan_start_pool_outcomes_enable(env.h, 1, None, _stream()), "deferred step sequence is open")
    refused(L.catan_start_pool_outcomes_read(env.h, op, 0, _stream()), "deferred step sequence is open")
    env.step_flush()
    # the host checks of the env's own methods
    for bad in ([1] * 63, [-1] + [1] * 63, [2 ** 32] + [0] * 63, [0] * 64, [2 ** 31, 2 ** 31] + [0] * 62):
        with pytest.raises(ValueError):
            env.set_start_pool_weights(bad)
    # ... and the weights in force are still the ones set at the start: a reset deals as the twin does
    twin.import_state(env.export_state().cpu().numpy())
    env.start_pool_counts(reset=True); twin.start_pool_counts(reset=True)           # (the deferred call may have re-dealt a game)
    env.reset(); twin.reset()
    _same_state(env, twin, "after the refusals")
    c = env.start_pool_counts()
    assert np.array_equal(c["per_entry"], twin.counts["per_entry"]) and all(c["per_entry"][k] == 0 for k in wr.ZEROS_64)
    # the largest sum is accepted
    env.set_start_pool_weights([2 ** 32 - 2, 1] + [0] * 62)


def test_collector_in_both_loops_with_balanced_sampling(hip_lib, pools):
    """RolloutCollector(start_pool_sampling="balanced") on the device loop and on the tensor-operation loop, the bot in every seat: the loops
    agree, storage.start_pool["outcomes"] is what the env tallied during the gather (read once, with reset), the tallied games are the
    finished ones, and after the second rollout the installed weights are balanced_weights of everything tallied - the second rollout's
    picks are those of the first rollout's balanced weights"""
    from settlers_of_catan_rl_amd import start_pool
    from settlers_of_catan_rl_amd.rollout import RolloutCollector
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy
    T, seen = 48, []
    for fused in (True, False):
        env = _env()
        bot = ScriptedPolicy(env)
        pool = start_pool.StartPool(pools[64])
        col = RolloutCollector(env, bot, T, opponents=[bot], seed=3, episode_stats=True, start_pool=pool, start_pool_fresh=0.25,
                               start_pool_sampling="balanced")
        col.fused_bookkeeping = fused
        assert col.start_pool_outcomes and col.start_pool is pool
        env.reset()
        env.start_pool_counts(reset=True)
        col.reset()
        installed = []
        inner_w = env.set_start_pool_weights
        env.set_start_pool_weights = lambda w: installed.append(np.array(w, copy=True)) or inner_w(w)
        reads = []
        inner = env.start_pool_outcomes
        env.start_pool_outcomes = lambda reset=False: reads.append(inner(reset)) or reads[-1]
        tables, per_entry = [], []
        for r in range(2):
            st = col.gather_rollouts()
            oc = st.start_pool["outcomes"]
            assert len(reads) == r + 1 and oc is reads[r]
            assert oc["seen"] == st.episode_stats["episodes"] == st.start_pool["pool"] + st.start_pool["fresh"] > 0 and oc["skipped"] == 0
            assert oc["focus_games"].sum() + oc["fresh"]["focus_games"] == st.episode_stats["focus_episodes"] == oc["seen"]
            assert oc["focus_wins"].sum() + oc["fresh"]["focus_wins"] == st.episode_stats["focus_wins"]
            tables.append(oc["table"].copy()); per_entry.append(st.start_pool["per_entry"].copy())
            assert not inner()["table"].any()
            col.after_rollouts()
        # the weights installed behind rollout r are balanced_weights of the tallies of rollouts 0..r
        first = start_pool.StartPool(pools[64]); first.add_outcomes(tables[0])
        assert len(installed) == 2 and np.array_equal(installed[0], first.balanced_weights())
        first.add_outcomes(tables[1])
        assert np.array_equal(installed[1], first.balanced_weights()) and np.array_equal(pool.outcomes, tables[0] + tables[1])
        assert len(set(installed[0].tolist())) > 1
        print("fused", fused, "tallied", int(tables[0][:, 0].sum()), int(tables[1][:, 0].sum()), "weights", int(installed[0].min()), int(installed[0].max()))
        seen.append((tables, per_entry, st.actions[:T].cpu(), st.rewards[:T].cpu(), st.masks[:T].cpu(), st.action_masks[:T].cpu()))
        assert env.invalid_action_count() == 0
    a, b = seen
    assert all(np.array_equal(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1]))
    assert all(torch.equal(x, y) for x, y in zip(a[2:], b[2:]))
