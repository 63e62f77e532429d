"""GPU: re-dealt games started from a pool of saved positions (csrc/catan_hooks.hip) - 64 games, so both 32-game
tiles of k_step with games 0, 31, 32 and 63, a global id base whose high and low words are both non-zero, the rule-based player in
every seat.  The twin is tests/start_pool_reference.py: the CPU oracle with the pick rule applied by export / import.  Every comparison
is integer (or bit) equality.  Seeds, pools and caps come from the reference module and are checked on the CPU by
tests/test_start_pool_cpu.py::test_seed_check_for_the_gpu_scenarios."""
import ctypes as C

import numpy as np
import pytest
import torch

import episode_stats_oracle as eso
import league_stats_oracle as lso
import record_reference as rr
import start_pool_reference as spr
from settlers_of_catan_rl_amd import record, spec

pytestmark = pytest.mark.gpu

N, SEED, ID0 = spr.N_GAMES, spr.SEED, spr.ENV_ID0
EINVAL = -1


@pytest.fixture(scope="module")
def pools():
    p = spr.pools()
    for v in p.values():
        v.setflags(write=False)
    return p


def _env(env_id0=ID0, auto_reset=True, n=N, **kw):
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    return VecCatanEnv(n, seed=SEED, env_id0=env_id0, auto_reset=auto_reset, **kw)


def _same_state(env, twin, where):
    got, want = env.export_state().cpu().numpy(), twin.blobs()
    for g in range(env.n):
        assert np.array_equal(got[g], want[g]), (where, g, spec.describe_state_diff(got[g], want[g]))
    assert np.array_equal(env.get_action_masks().cpu().numpy(), twin.masks()), where


def _same_counts(env, twin):
    c, w = env.start_pool_counts(), twin.counts
    assert (c["pool"], c["fresh"]) == (w["pool"], w["fresh"]) and np.array_equal(c["per_entry"], w["per_entry"]), (c, w)
    assert c["pool"] + c["fresh"] == int(twin.deals.sum())
    return c


def _lockstep(env, twin, steps):
    """reset() under the pool, then `steps` steps with the device's scripted sampler; after every step all blobs, mask rows, rewards and
    done flags equal the twin's, which is fed the same action rows"""
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
    assert env.invalid_action_count() == 0 and env.missed_speculation_count() == 0


@pytest.mark.parametrize("m,env_id0", [(1, spr.ENV_ID0_ZERO), (3, ID0), (64, ID0)])
def test_lockstep_equals_the_twin(hip_lib, pools, m, env_id0):
    """(1) catan_step with pools of 1, 3 and 64 entries, every deal from the pool"""
    env, twin = _env(env_id0), spr.PoolTwin(N, SEED, env_id0, pools[m], 0)
    env.set_start_pool(pools[m])
    _lockstep(env, twin, spr.STEP_CAP)
    c = _same_counts(env, twin)
    print("pool", m, "deals", c["pool"], "games dealt three times or more", int((twin.deals >= 3).sum()))
    assert c["fresh"] == 0 and c["pool"] >= 64 + 32 and (twin.deals >= 3).any()
    if m <= 3:
        assert (c["per_entry"] > 0).all()


def test_half_fresh_equals_the_twin(hip_lib, pools):
    """(2) fresh_q16 = 32 768 with the 3-entry pool"""
    env, twin = _env(), spr.PoolTwin(N, SEED, ID0, pools[3], 32768)
    env.set_start_pool(torch.from_numpy(pools[3].copy()), fresh_share=0.5)
    _lockstep(env, twin, spr.STEP_CAP)
    c = _same_counts(env, twin)
    assert c["pool"] >= 8 and c["fresh"] >= 8, c


def test_all_fresh_equals_an_env_without_a_pool(hip_lib, pools):
    """(3) fresh_q16 = 65 536 against a second env that never had a pool, both started from the same late positions so that games end:
    identical blobs, masks, rewards and done at every step, and every deal is counted under `fresh`"""
    a, b = _env(), _env()
    a.set_start_pool(pools[3], fresh_share=1.0)
    for e in (a, b):
        e.reset()
        e.import_state(pools[64].copy())
    deals = N
    for t in range(150):
        ra, da = a.step(a.sample_scripted_actions())
        rb, db = b.step(b.sample_scripted_actions())
        assert torch.equal(ra, rb) and torch.equal(da, db), t
        assert torch.equal(a.export_state(), b.export_state()) and torch.equal(a.get_action_masks(), b.get_action_masks()), t
        deals += int(da.sum())
    c = a.start_pool_counts()
    assert deals > N and (c["pool"], c["fresh"]) == (0, deals) and not c["per_entry"].any(), (c, deals)


def _deferred(env, twin, calls, window):
    """step_deferred with the bot, then the flush.  A call's action is applied iff the game was not WAITING after the previous call (and it
    is no no-op); the twin gets exactly the applied rows (a no-op for every other game), so it holds each game's own sequence of
    completed steps.  A result is delivered with the game's next status 0: it must be the twin's for that step."""
    waiting, outstanding = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
    want_r, want_d = np.zeros((N, 4), dtype=np.float32), np.zeros(N, dtype=np.uint8)
    delivered_total = 0

    def deliver(r_h, d_h, sel):
        nonlocal delivered_total
        assert np.array_equal(r_h[sel], want_r[sel]) and np.array_equal(d_h[sel], want_d[sel])
        delivered_total += int(sel.sum())

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
    return delivered_total


@pytest.mark.parametrize("window", [1, 4])
def test_deferred_equals_the_twin(hip_lib, pools, window):
    """(4) catan_step_deferred, flushed at the end: per game the sequence of completed steps (reward, done) and the final blobs and masks
    equal the twin's, and the counters equal those of the twin - a lock-step run of the same per-game step counts"""
    env, twin = _env(), spr.PoolTwin(N, SEED, ID0, pools[3], 0)
    env.set_start_pool(pools[3])
    env.reset(); twin.reset()
    delivered = _deferred(env, twin, spr.STEP_CAP, window)
    _same_state(env, twin, "after the flush")
    c = _same_counts(env, twin)
    print("window", window, "delivered steps", delivered, "deals", c["pool"])
    assert c["pool"] > 64 + 16 and env.invalid_action_count() == 0


def test_random_rollout_equals_the_twin(hip_lib, oracle, pools):
    """(5) catan_random_rollout (lock-step, the library's uniform-random policy) with the 3-entry pool: the twin is stepped with the actions
    the oracle's sampler draws for (seed, game id, step index) - the ones the library draws, as the parity tests rely on"""
    env, twin = _env(), spr.PoolTwin(N, SEED, ID0, pools[3], 0)
    env.set_start_pool(pools[3])
    env.reset(); twin.reset()
    env.random_rollout(0, spr.RANDOM_STEPS)
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    for s in range(spr.RANDOM_STEPS):
        masks, a = twin.masks(), np.zeros((N, 18), dtype=np.int32)
        for g in range(N):
            twin.L.orc_sample_action(twin.b.env_ptr(g), SEED, ID0 + g, s, masks[g].ctypes.data_as(f32p), a[g].ctypes.data_as(i32p))
        twin.step(torch.from_numpy(a))
    _same_state(env, twin, "after the rollout")
    c = _same_counts(env, twin)
    assert c["pool"] > 64, c


def test_reset_with_a_mask_and_without(hip_lib, pools):
    """(6) catan_reset: the selected games equal their pool entry apart from rng_draws, the others are untouched; NULL means every game"""
    env, twin = _env(), spr.PoolTwin(N, SEED, ID0, pools[3], 0)
    env.set_start_pool(pools[3])
    before = env.export_state().cpu().numpy()
    sel = np.zeros(N, dtype=bool)
    sel[[0, 5, 31, 32, 63]] = True
    env.reset(torch.from_numpy(sel)); twin.reset(sel)
    _same_state(env, twin, "after the masked reset")
    after = env.export_state().cpu().numpy()
    entries = {spr._zero_rng(b) for b in pools[3]}
    for g in range(N):
        if sel[g]:
            assert spr._zero_rng(after[g]) in entries and after[g][spr.RNG_WORD] != before[g][spr.RNG_WORD], g
        else:
            assert np.array_equal(after[g], before[g]), g
    assert _same_counts(env, twin)["pool"] == 5
    env.reset(); twin.reset()
    _same_state(env, twin, "after the full reset")
    after = env.export_state().cpu().numpy()
    assert all(spr._zero_rng(after[g]) in entries for g in range(N))
    assert _same_counts(env, twin)["pool"] == 5 + N


def test_clear_makes_every_deal_fresh_again(hip_lib, pools):
    """(7) after clear_start_pool() the next re-deals equal those of an env that imported this env's states and never had a pool"""
    from settlers_of_catan_rl_amd._lib import CatanHipError
    a, b = _env(), _env()
    a.set_start_pool(pools[64])
    a.reset()
    for _ in range(20):
        a.step(a.sample_scripted_actions())
    a.clear_start_pool()
    with pytest.raises(CatanHipError):
        a.start_pool_counts()
    b.import_state(a.export_state())
    dones = 0
    for t in range(150):
        ra, da = a.step(a.sample_scripted_actions())
        rb, db = b.step(b.sample_scripted_actions())
        assert torch.equal(ra, rb) and torch.equal(da, db), t
        assert torch.equal(a.export_state(), b.export_state()) and torch.equal(a.get_action_masks(), b.get_action_masks()), t
        dones += int(da.sum())
    assert dones >= 8
    a.clear_start_pool()                                     # without a pool: nothing to do


def test_a_second_set_replaces_the_pool_and_zeroes_the_counters(hip_lib, pools):
    """(8)"""
    env, twin = _env(), spr.PoolTwin(N, SEED, ID0, pools[1], 0)
    env.set_start_pool(pools[1])
    env.reset(); twin.reset()
    c = _same_counts(env, twin)
    assert c["pool"] == N and c["per_entry"].tolist() == [N]
    env.set_start_pool(pools[3], fresh_share=0.25)
    twin.set_pool(pools[3], 16384); twin.deals[:] = 0
    c = env.start_pool_counts()
    assert (c["pool"], c["fresh"], c["per_entry"].tolist()) == (0, 0, [0, 0, 0])
    env.reset(); twin.reset()
    _same_state(env, twin, "after the reset under the second pool")
    c = _same_counts(env, twin)
    assert c["pool"] + c["fresh"] == N and c["fresh"] > 0 and c["per_entry"].shape == (3,)
    assert env.start_pool_counts(reset=True)["pool"] == c["pool"] and env.start_pool_counts()["pool"] == 0


def test_a_record_armed_at_the_deal_starts_from_the_installed_position(hip_lib, pools):
    """(9) every game has a record slot armed at_deal: a sealed record's start blob is the state the twin's deal left - the installed position
    with the game's own rng_draws -, FROM_DEAL is set, and the oracle replay reaches the final blob"""
    env, twin = _env(), spr.PoolTwin(N, SEED, ID0, pools[3], 0)
    env.set_start_pool(pools[3])
    env.reset(); twin.reset()
    env.enable_recording(list(range(N)), capacity=spr.STEP_CAP)
    env.arm_recording(at_deal=True)
    twin.deal_log.clear()
    for t in range(spr.STEP_CAP):
        a = env.sample_scripted_actions()
        a_h = a.cpu().numpy()
        env.step(a)
        twin.step(torch.from_numpy(a_h))
    first_deal = {}
    for g, blob in twin.deal_log:
        first_deal.setdefault(g, blob)
    recs = env.recordings()
    print(len(recs), "sealed records")
    assert len(recs) >= 8
    entries = {spr._zero_rng(b) for b in pools[3]}
    for rec in recs:
        g = rec.game_id - ID0
        assert rec.from_deal and not rec.truncated and rec.seed == SEED
        assert np.array_equal(rec.start_blob, first_deal[g]) and spr._zero_rng(rec.start_blob) in entries, g
        final, _rew, done, rejected = rr.replay_on_cpu(rec.seed, rec.game_id, rec.start_blob, rec.actions, **rec.cfg)
        assert np.array_equal(final, rec.final_blob) and done[-1] and not done[:-1].any() and not rejected.any(), g
    steps = list(record.replay(recs[0]))                     # product code: a one-game env on the device
    assert np.array_equal(steps[-1][5], recs[0].final_blob)


def _episodes(finished):
    """the twin's finished games as rows of episode_stats_oracle.replay (DECISION 0: inside every counter)"""
    rows = []
    for g, blob in finished:
        f = lambda name: spec.state_field(blob, name)
        rows.append([g, 0, int(f("winner")[0]), int(f("turn")[0]), int(f("lr_player")[0]), int(f("la_player")[0])]
                    + [int(f(f"p{p}_vp")[0]) for p in (1, 2, 3, 4)] + [int(x) for x in f("player_order")]
                    + [int(x) for x in f("settlements_left")] + [int(x) for x in f("cities_left")]
                    + [int(f(f"p{p}_n_played")[0]) for p in (1, 2, 3, 4)])
    return np.array(rows, dtype=np.int64).reshape(-1, eso.COLS)


def test_finished_game_statistics_and_league_table_count_pool_games(hip_lib, pools):
    """(10) both tallies on: their tables equal the two plain-Python oracles run over the twin's finished games (a pool-started game's
    turns include the turns its position already had)"""
    num_nets = 3
    env, twin = _env(), spr.PoolTwin(N, SEED, ID0, pools[64], 0)
    slot, net = lso.maps(N, num_nets, 4)
    focus = (np.arange(N) % 5).astype(np.int32)
    env.set_start_pool(pools[64])
    env.enable_episode_stats(torch.from_numpy(focus))
    env.enable_league_stats(torch.from_numpy(slot), torch.from_numpy(net), num_nets)
    _lockstep(env, twin, spr.STEP_CAP)
    ep = _episodes(twin.finished)
    assert len(ep) >= 32
    want = eso.counters(ep, 0, focus)
    got = env.episode_stats_words()
    assert got == want, (eso.named(got), eso.named(want))
    assert np.array_equal(env.league_stats().numpy(), lso.table(ep, 0, slot, net, num_nets))


def test_error_returns_leave_the_installed_pool_intact(hip_lib, pools):
    """(11) every CATAN_EINVAL of the interface; the pool installed before stays as it was"""
    from settlers_of_catan_rl_amd.env import VecCatanEnv, _ptr, _stream
    L = hip_lib
    dev = torch.device("cuda")
    env, twin = _env(), spr.PoolTwin(N, SEED, ID0, pools[3], 0)
    env.set_start_pool(pools[3])
    good = torch.from_numpy(pools[64].copy()).to(dev).t().contiguous()          # [736][64]
    out = np.zeros(2 + 3, dtype=np.uint64)
    op = out.ctypes.data_as(C.POINTER(C.c_uint64))

    def refused(rc, word):
        assert rc == EINVAL and word.encode() in L.catan_last_error(), (rc, L.catan_last_error())
        assert L.catan_start_pool_size(env.h) == 3

    refused(L.catan_start_pool_set(None, _ptr(good), 64, 0, _stream()), "null handle")
    refused(L.catan_start_pool_set(env.h, None, 64, 0, _stream()), "null blobs")
    refused(L.catan_start_pool_set(env.h, _ptr(good), 0, 0, _stream()), "m must be in")
    refused(L.catan_start_pool_set(env.h, _ptr(good), 65537, 0, _stream()), "m must be in")
    refused(L.catan_start_pool_set(env.h, _ptr(good), 64, 65537, _stream()), "fresh_q16 must be in")
    refused(L.catan_start_pool_set(env.h, _ptr(good), 64, -1, _stream()), "fresh_q16 must be in")
    refused(L.catan_start_pool_read(env.h, None, 0, _stream()), "null argument")
    with pytest.raises(ValueError):
        env.set_start_pool(pools[3], fresh_share=1.5)
    with pytest.raises(ValueError):
        env.set_start_pool(pools[3][:, :700])
    # a finished blob among valid ones (checked on the device)
    bad = pools[64].copy()
    spec.state_field(bad[17], "winner")[...] = 2
    refused(L.catan_start_pool_set(env.h, _ptr(torch.from_numpy(bad).to(dev).t().contiguous()), 64, 0, _stream()), "finished games")
    # a handle under the MT19937 contract
    one = VecCatanEnv(1, seed=3, auto_reset=False)
    one.seed_mt19937(1, 2)
    refused(L.catan_start_pool_set(one.h, _ptr(good), 64, 0, _stream()), "MT19937")
    assert L.catan_start_pool_size(one.h) == 0
    # an open deferred sequence: set, clear and read
    env.step_deferred(env.sample_scripted_actions(), window=4)
    refused(L.catan_start_pool_set(env.h, _ptr(good), 64, 0, _stream()), "deferred step sequence is open")
    refused(L.catan_start_pool_clear(env.h, _stream()), "deferred step sequence is open")
    refused(L.catan_start_pool_read(env.h, op, 0, _stream()), "deferred step sequence is open")
    env.step_flush()
    # the library's own deferred rollout while a pool is installed, in both of its forms, and its timed form
    ms = (C.c_float * 5)()
    for fused in (True, False):
        env.set_deferred_fused(fused)
        refused(L.catan_random_rollout_deferred(env.h, 8, 4, _stream()), "start pool is installed")
        refused(L.catan_random_rollout_timed(env.h, 0, 8, 4, _stream(), ms), "start pool is installed")
    # ... and the pool is the one installed at the start: a reset deals from it as the twin does
    twin.import_state(env.export_state().cpu().numpy())
    env.reset(); twin.reset()
    _same_state(env, twin, "after the refusals")
    c = env.start_pool_counts()
    assert (c["pool"], c["fresh"]) == (N, 0) and np.array_equal(c["per_entry"], twin.counts["per_entry"])
    # without a pool: read is refused, the deferred rollout runs
    env.clear_start_pool()
    assert L.catan_start_pool_read(env.h, op, 0, _stream()) == EINVAL and b"no start pool" in L.catan_last_error()
    env.random_rollout_deferred(8, 4)


def test_a_refused_set_leaves_the_pool_of_two_that_steps_install_from(hip_lib, pools):
    """(11b) the new pool is built beside the one in use: a set of 4 blobs with a finished game among them is refused on the device, and
    the pool of 2 installed before is still what catan_start_pool_size and catan_start_pool_read report and what the re-deals of the
    following catan_step calls install from, as the twin's do"""
    from settlers_of_catan_rl_amd.env import _ptr, _stream
    two, four = pools[64][:2], pools[64][2:6].copy()
    spec.state_field(four[1], "winner")[...] = 3
    env, twin = _env(), spr.PoolTwin(N, SEED, ID0, two, 0)
    env.set_start_pool(two)
    bad = torch.from_numpy(four).to(env.device).t().contiguous()
    assert hip_lib.catan_start_pool_set(env.h, _ptr(bad), 4, 0, _stream()) == EINVAL and b"1 blobs are positions of finished games" in hip_lib.catan_last_error()
    assert hip_lib.catan_start_pool_size(env.h) == 2
    c = env.start_pool_counts()
    assert (c["pool"], c["fresh"], c["per_entry"].tolist()) == (0, 0, [0, 0])
    _lockstep(env, twin, spr.REFUSED_SET_STEPS)
    c = _same_counts(env, twin)
    print("installs behind the refused set", c["pool"], c["per_entry"].tolist())
    assert c["pool"] > N and c["fresh"] == 0 and c["per_entry"].shape == (2,)


def test_collector_in_both_loops(hip_lib, pools):
    """(12) RolloutCollector(start_pool=...) on the device loop (_gather_device) and on the tensor-operation loop (_gather_tensor), the bot in
    every seat: the loops agree with each other, storage.start_pool is what the env counted during the gather (read with reset), and
    every finished game was dealt once"""
    from settlers_of_catan_rl_amd.rollout import RolloutCollector
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy
    T, seen = 48, []
    for fused in (True, False):
        env = _env()
        bot = ScriptedPolicy(env)
        col = RolloutCollector(env, bot, T, opponents=[bot], seed=3, episode_stats=True, start_pool=pools[64], start_pool_fresh=0.25)
        col.fused_bookkeeping = fused
        env.reset()
        first = env.start_pool_counts(reset=True)
        assert first["pool"] + first["fresh"] == N and first["fresh"] > 0
        col.reset()
        reads = []
        inner = env.start_pool_counts
        env.start_pool_counts = lambda reset=False: reads.append(inner(reset)) or reads[-1]
        st = col.gather_rollouts()
        assert len(reads) == 1 and st.start_pool is reads[0]
        sp = st.start_pool
        print("fused", fused, "pool", sp["pool"], "fresh", sp["fresh"], "episodes", st.episode_stats["episodes"])
        assert sp["pool"] + sp["fresh"] == st.episode_stats["episodes"] > 0
        after = inner()
        assert after["pool"] == after["fresh"] == 0 and not after["per_entry"].any()
        seen.append((sp, st.actions[:T].cpu(), st.rewards[:T].cpu(), st.masks[:T].cpu(), st.action_masks[:T].cpu()))
        assert env.invalid_action_count() == 0
    a, b = seen
    assert (a[0]["pool"], a[0]["fresh"]) == (b[0]["pool"], b[0]["fresh"]) and np.array_equal(a[0]["per_entry"], b[0]["per_entry"])
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))


def test_evaluator_starts_every_game_from_its_blob(hip_lib, pools):
    """(13) run_evaluation_episodes(start_blobs=...): game g's first observed state is blob g % len (the record's start blob), and two runs
    with the same seeds are identical"""
    import random
    from settlers_of_catan_rl_amd import evaluation as ev
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy
    n = 16

    def run(**kw):
        env = _env(env_id0=100, auto_reset=False, n=n)
        bot = ScriptedPolicy(env)
        return env, ev.run_evaluation_episodes(env, [bot, bot, bot, bot], ev.sample_orders(n, random.Random(2)), max_steps=2500, **kw)
    _, plain = run()
    env1, r1 = run(start_blobs=pools[3], record=n)
    env2, r2 = run(start_blobs=torch.from_numpy(pools[3].copy()), record=n)
    assert list(r1) == list(plain) + ["records"]
    for g, rec in enumerate(r1["records"]):
        assert np.array_equal(rec.start_blob, pools[3][g % 3]), g
        assert rec.final_blob is not None and rec.length == int(r1["game_steps"][g])
    assert all(np.array_equal(r1[k], r2[k]) for k in plain)
    assert all(a == b for a, b in zip(r1["records"], r2["records"]))
    assert torch.equal(env1.export_state(), env2.export_state())
    assert not np.array_equal(r1["game_steps"], plain["game_steps"])
