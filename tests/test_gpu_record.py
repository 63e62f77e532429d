"""GPU: whole games recorded on the device (csrc/catan_hooks.hip) - 64 games, 16 slots on both 32-game tiles of k_step
(games 0, 31, 32 and 63 among them), the rule-based player in every seat.  Everything is compared with integer equality; a replay steps the
record's start blob through oracle/libcatan_cpu.so created with n = 1, the record's seed and env_id0 = the game id.  The seed and the
step caps come from tests/record_reference.py and are checked on the CPU by tests/test_record_cpu.py, so every armed slot must seal."""
import ctypes as C

import numpy as np
import pytest
import torch

import record_reference as rr
from settlers_of_catan_rl_amd import record, spec

pytestmark = pytest.mark.gpu

N, SEED, GAMES = rr.N_GAMES, rr.SEED, rr.ARMED_GAMES
EINVAL = -1
WINDOW = 4


def _env(auto_reset, **kw):
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    return VecCatanEnv(N, seed=SEED, env_id0=rr.ENV_ID0, auto_reset=auto_reset, **kw)


def _replay_checks(rec, live_reward=None, live_done=None):
    """the oracle replay of a sealed record reaches its final blob, done on the last action only -> the replay's rejected flags"""
    final, rew, done, rejected = rr.replay_on_cpu(rec.seed, rec.game_id, rec.start_blob, rec.actions, **rec.cfg)
    assert np.array_equal(final, rec.final_blob), (rec.game_id, spec.describe_state_diff(final, rec.final_blob))
    assert done[-1] and not done[:-1].any(), rec.game_id
    assert int(spec.state_field(rec.final_blob, "winner")[0]) in (1, 2, 3, 4)
    if live_reward is not None:
        assert np.array_equal(rew, np.array(live_reward, dtype=np.float32).reshape(-1, 4)), rec.game_id
        assert done.tolist() == [bool(d) for d in live_done], rec.game_id
    return rejected


def _status(env):
    return env.recording_status().numpy()


def test_lockstep_no_auto_reset_armed_now(hip_lib):
    """(a) every armed game from its reset to its end; game 5 is frozen (no-op) every seventh step, finished games get the no-op"""
    env = _env(False)
    env.enable_recording(GAMES, capacity=rr.STEP_CAP_ONE)
    env.arm_recording()
    start = env.export_state().cpu().numpy()
    finished = torch.zeros(N, dtype=torch.bool, device=env.device)
    fin_h = np.zeros(N, dtype=bool)
    passed, live_r, live_d, final = {g: [] for g in GAMES}, {g: [] for g in GAMES}, {g: [] for g in GAMES}, {}
    for t in range(rr.STEP_CAP_ONE + rr.STEP_CAP_ONE // 6):          # (game 5 sits out every seventh step)
        a = env.sample_scripted_actions().clone()
        a[finished, 0] = -1
        if t % 7 == 6:
            a[5, 0] = -1
        a_h = a.cpu().numpy()
        reward, done = env.step(a)
        r_h, d_h = reward.cpu().numpy(), done.cpu().numpy().astype(bool)
        for g in GAMES:
            if a_h[g, 0] >= 0:
                passed[g].append(a_h[g]); live_r[g].append(r_h[g].copy()); live_d[g].append(d_h[g])
                if d_h[g]:
                    final[g] = env.export_state([g])[0].cpu().numpy()
        finished |= done.bool()
        fin_h |= d_h
        if fin_h[GAMES].all():
            break
    assert fin_h[GAMES].all(), "the step cap of tests/test_record_cpu.py was not enough"
    st = _status(env)
    assert (st[:, 0] == record.SEALED).all() and st[:, 1].tolist() == GAMES and (st[:, 3] == 0).all(), st
    recs = env.recordings()
    assert len(recs) == len(GAMES) and env.invalid_action_count() == 0
    for s, (g, rec) in enumerate(zip(GAMES, recs)):
        assert (rec.seed, rec.game_id, rec.length) == (SEED, rr.ENV_ID0 + g, len(passed[g])) and not rec.truncated and not rec.from_deal
        assert int(st[s, 2]) == len(passed[g])
        assert np.array_equal(rec.actions, np.array(passed[g])), g
        assert np.array_equal(rec.start_blob, start[g]) and np.array_equal(rec.final_blob, final[g]), g
        assert not _replay_checks(rec, live_r[g], live_d[g]).any()


def _check_from_deal(rec, g, first_start, logged):
    assert rec.from_deal and not rec.truncated and rec.game_id == rr.ENV_ID0 + g
    f = lambda blob, name: spec.state_field(blob, name)
    assert int(f(rec.start_blob, "rng_draws")[0]) != int(f(first_start[g], "rng_draws")[0])
    assert not (np.array_equal(f(rec.start_blob, "tile_res"), f(first_start[g], "tile_res"))
                and np.array_equal(f(rec.start_blob, "tile_val"), f(first_start[g], "tile_val"))), g
    assert int(f(rec.start_blob, "turn")[0]) == 0 and int(f(rec.start_blob, "winner")[0]) == 0
    assert rec.length == len(logged) and np.array_equal(rec.actions, np.array(logged)), g
    assert not _replay_checks(rec).any()


def test_lockstep_auto_reset_armed_at_deal(hip_lib):
    """(b) the first episode of every armed game passes unrecorded (WAIT_DEAL, length 0, until its done is seen), the second is recorded"""
    env = _env(True)
    env.enable_recording(GAMES, capacity=rr.STEP_CAP_TWO)
    env.arm_recording(at_deal=True)
    first_start = env.export_state().cpu().numpy()
    episodes = np.zeros(N, dtype=np.int64)
    logged = {g: [] for g in GAMES}
    for t in range(rr.STEP_CAP_TWO):
        st = _status(env)
        for s, g in enumerate(GAMES):
            if episodes[g] == 0:
                assert st[s, 0] == record.WAIT_DEAL and st[s, 2] == 0, (t, g, st[s])
            elif episodes[g] == 1:
                assert st[s, 0] == record.RECORDING and st[s, 2] == len(logged[g]) and st[s, 3] == record.F_FROM_DEAL, (t, g, st[s])
        a = env.sample_scripted_actions()
        a_h = a.cpu().numpy()
        _, done = env.step(a)
        d_h = done.cpu().numpy().astype(bool)
        for g in GAMES:
            if episodes[g] == 1:
                logged[g].append(a_h[g])
        episodes += d_h
        if (episodes[GAMES] >= 2).all():
            break
    assert (episodes[GAMES] >= 2).all(), "the step cap of tests/test_record_cpu.py was not enough"
    st = _status(env)
    assert (st[:, 0] == record.SEALED).all(), st
    for g, rec in zip(GAMES, env.recordings()):
        _check_from_deal(rec, g, first_start, logged[g])
    assert env.invalid_action_count() == 0 and env.missed_speculation_count() == 0


def _deferred_run(env, n_done, cap, skip_first_episode):
    """step_deferred with the bot until every armed game has delivered n_done done flags, then the flush.  The action of a call is applied
    iff the game's status from the previous call was not WAITING (and it is no no-op); its result arrives with the game's next status 0.
    -> (applied rows per armed game, for the episode that is recorded; live rewards; live dones)"""
    waiting = np.zeros(N, dtype=bool)
    episodes = np.zeros(N, dtype=np.int64)
    out = {g: [] for g in GAMES}; live_r = {g: [] for g in GAMES}; live_d = {g: [] for g in GAMES}
    outstanding = np.zeros(N, dtype=bool)            # an applied action whose result has not been delivered
    rec_ep = 1 if skip_first_episode else 0
    stop_at = None
    for t in range(cap):
        a = env.sample_scripted_actions().clone()
        if not env.cfg.auto_reset:
            a[torch.from_numpy(episodes > 0).to(env.device), 0] = -1
        a_h = a.cpu().numpy()
        applied = ~waiting & (a_h[:, 0] >= 0)
        for g in GAMES:
            if applied[g] and episodes[g] == rec_ep:
                out[g].append(a_h[g])
        outstanding |= applied
        reward, done, status = env.step_deferred(a, window=WINDOW)
        r_h, d_h, s_h = reward.cpu().numpy(), done.cpu().numpy().astype(bool), status.cpu().numpy()
        delivered = (s_h == 0) & outstanding
        for g in GAMES:
            if delivered[g] and episodes[g] == rec_ep:
                live_r[g].append(r_h[g].copy()); live_d[g].append(d_h[g])
        episodes += delivered & d_h
        outstanding &= ~delivered
        waiting = s_h == 1
        if (episodes[GAMES] >= n_done).all():
            stop_at = t
            break
    assert stop_at is not None, "the call cap was not enough"
    reward, done, status = env.step_flush()
    r_h, d_h, s_h = reward.cpu().numpy(), done.cpu().numpy().astype(bool), status.cpu().numpy()
    assert ((s_h == 0) == waiting).all()
    for g in GAMES:
        if waiting[g] and outstanding[g] and episodes[g] == rec_ep:
            live_r[g].append(r_h[g].copy()); live_d[g].append(d_h[g])
    return out, live_r, live_d


def test_deferred_no_auto_reset_armed_now(hip_lib):
    """(c) step_deferred with window 4 to every armed game's end, then the flush: the log is what was applied (a waiting game's row is
    not), the final blob is the export after the flush, the replay gives every delivered reward and done flag"""
    env = _env(False)
    env.enable_recording(GAMES, capacity=rr.STEP_CAP_ONE)
    env.arm_recording()
    start = env.export_state().cpu().numpy()
    applied, live_r, live_d = _deferred_run(env, 1, 6 * rr.STEP_CAP_ONE, False)
    final = env.export_state().cpu().numpy()                     # (no re-deal: the finished games stay where they ended)
    st = _status(env)
    assert (st[:, 0] == record.SEALED).all() and (st[:, 3] == 0).all(), st
    for g, rec in zip(GAMES, env.recordings()):
        assert rec.length == len(applied[g]) and np.array_equal(rec.actions, np.array(applied[g])), g
        assert np.array_equal(rec.start_blob, start[g]) and np.array_equal(rec.final_blob, final[g]), g
        assert len(live_d[g]) == rec.length
        assert not _replay_checks(rec, live_r[g], live_d[g]).any()
    assert env.invalid_action_count() == 0


def test_deferred_auto_reset_armed_at_deal_then_flush(hip_lib):
    """(d) as (c) with auto-reset: the first episode passes unrecorded, the second is recorded from its deal on the window's side stream
    and sealed there; the checks of (b)"""
    env = _env(True)
    env.enable_recording(GAMES, capacity=rr.STEP_CAP_TWO)
    env.arm_recording(at_deal=True)
    first_start = env.export_state().cpu().numpy()
    assert (_status(env)[:, 0] == record.WAIT_DEAL).all()
    applied, _, _ = _deferred_run(env, 2, 6 * rr.STEP_CAP_TWO, True)
    st = _status(env)
    assert (st[:, 0] == record.SEALED).all(), st
    for g, rec in zip(GAMES, env.recordings()):
        _check_from_deal(rec, g, first_start, applied[g])
    assert env.invalid_action_count() == 0


def test_overflow_keeps_the_first_actions_and_counts_on(hip_lib):
    """(e) capacity 64, 100 steps: nothing is written past the log (the guard word behind every slot's log is intact), TRUNCATED is set, the
    length is the true count"""
    cap, steps = rr.OVERFLOW_CAPACITY, 100
    env = _env(False)
    env.enable_recording(GAMES, capacity=cap)
    env.arm_recording()
    passed = []
    for t in range(steps):
        a = env.sample_scripted_actions()
        passed.append(a.cpu().numpy())
        env.step(a)
        if t == cap - 1:
            assert (_status(env)[:, 2:] == [cap, 0]).all()       # full, not yet truncated
    st = _status(env)
    assert (st[:, 0] == record.RECORDING).all() and (st[:, 2] == steps).all() and (st[:, 3] == record.F_TRUNCATED).all(), st
    assert env.recordings() == []                                # none is sealed
    recs = env.recordings(sealed_only=False)
    passed = np.stack(passed, 1)                                 # [N, steps, 18]
    for g, rec in zip(GAMES, recs):
        assert rec.truncated and rec.length == steps and rec.final_blob is None and rec.actions.shape == (cap, 18)
        assert np.array_equal(rec.actions, passed[g, :cap]), g
    lines = record.describe(recs[0], env=rr.CpuEnv(recs[0].seed, recs[0].game_id, **recs[0].cfg))
    assert len(lines) == cap + 2 and lines[-1] == f"truncated: the first {cap} of {steps} actions were kept"


def test_a_rejected_action_is_logged_and_rejected_again(hip_lib):
    """(f) validate_actions on: a dice roll in the placement phase, games 0 and 31, between bot moves"""
    env = _env(False, validate_actions=True)
    env.enable_recording(GAMES, capacity=64)
    env.arm_recording()
    passed = []
    for t in range(11):
        a = env.sample_scripted_actions().clone()
        if t == 5:
            a[0] = 0; a[31] = 0
            a[0, 0] = 9; a[31, 0] = 9
        passed.append(a.cpu().numpy())
        env.step(a)
    assert env.invalid_action_count() == 2
    passed = np.stack(passed, 1)
    live = env.export_state().cpu().numpy()
    for g, rec in zip(GAMES, env.recordings(sealed_only=False)):
        assert rec.length == 11 and np.array_equal(rec.actions, passed[g]), g
        final, _, done, rejected = rr.replay_on_cpu(rec.seed, rec.game_id, rec.start_blob, rec.actions, **rec.cfg)
        assert rejected.tolist() == [g in (0, 31) and t == 5 for t in range(11)], g
        assert np.array_equal(final, live[g]) and not done.any(), g


def _plain_run(deferred, recording):
    env = _env(True)
    if recording:
        env.enable_recording(GAMES, capacity=128)
        env.arm_recording(slots=list(range(0, 16, 2)))
        env.arm_recording(slots=list(range(1, 16, 2)), at_deal=True)
    rewards = []
    for t in range(320):
        a = env.sample_scripted_actions()
        if deferred:
            r, d, s = env.step_deferred(a, window=WINDOW)
            rewards.append(torch.cat((r, d[:, None].float(), s[:, None].float()), 1).clone())
        else:
            r, d = env.step(a)
            rewards.append(torch.cat((r, d[:, None].float()), 1).clone())
    if deferred:
        r, d, s = env.step_flush()
        rewards.append(torch.cat((r, d[:, None].float(), s[:, None].float()), 1).clone())
    return env.export_state().cpu().numpy(), torch.stack(rewards).cpu().numpy(), env.invalid_action_count()


@pytest.mark.parametrize("deferred", [False, True])
def test_recording_does_not_perturb_the_games(hip_lib, deferred):
    """(g) two identical runs of 320 calls, recording off and on (half the slots armed now, half at the deal, logs overflowing): the
    same states, rewards, done flags, statuses and invalid-action count"""
    off, on = _plain_run(deferred, False), _plain_run(deferred, True)
    assert np.array_equal(off[0], on[0]) and np.array_equal(off[1], on[1]) and off[2] == on[2]


def test_error_returns(hip_lib):
    """(h) every CATAN_EINVAL of the interface, nothing launched"""
    from settlers_of_catan_rl_amd.env import VecCatanEnv, _ptr, _stream
    from settlers_of_catan_rl_amd._lib import CatanHipError
    L = hip_lib
    dev = torch.device("cuda")
    games = torch.tensor(GAMES, dtype=torch.int32, device=dev)
    status = np.zeros((16, 4), dtype=np.uint32)
    sp = status.ctypes.data_as(C.c_void_p)
    hdr = np.zeros(4, dtype=np.uint32)
    hp = hdr.ctypes.data_as(C.c_void_p)
    slots = np.arange(4, dtype=np.int32)

    def refused(rc, word):
        assert rc == EINVAL and word.encode() in L.catan_last_error(), (rc, L.catan_last_error())

    # a null handle
    refused(L.catan_record_enable(None, _ptr(games), 16, 64, _stream()), "null handle")
    refused(L.catan_record_arm(None, None, 0, record.RECORD_NOW, _stream()), "null handle")
    refused(L.catan_record_status(None, sp, _stream()), "null argument")
    refused(L.catan_record_read(None, 0, None, None, None, hp, _stream()), "null argument")
    env, plain = _env(True), _env(False)
    with pytest.raises(CatanHipError):
        env.recordings()                                                                       # while off
    with pytest.raises(CatanHipError):
        env.recording_status()
    # arm, status, read while recording is not enabled
    refused(L.catan_record_arm(env.h, None, 0, record.RECORD_NOW, _stream()), "not enabled")
    refused(L.catan_record_status(env.h, sp, _stream()), "not enabled")
    refused(L.catan_record_read(env.h, 0, None, None, None, hp, _stream()), "not enabled")
    # m and capacity out of range
    for m, cap in ((-1, 64), (4097, 64), (16, 0), (16, 65536)):
        refused(L.catan_record_enable(env.h, _ptr(games), m, cap, _stream()), "must be in")
    refused(L.catan_record_enable(env.h, None, 16, 64, _stream()), "null games")
    # a game id outside [0, n), a game listed twice: checked on the device, nothing stays enabled
    for bad in ([0, 1, N], [0, -1, 2], [3, 4, 3]):
        refused(L.catan_record_enable(env.h, _ptr(torch.tensor(bad, dtype=torch.int32, device=dev)), 3, 64, _stream()), "outside [0, n)")
        refused(L.catan_record_status(env.h, sp, _stream()), "not enabled")
    # a handle under the MT19937 contract
    one = VecCatanEnv(1, seed=3, auto_reset=False)
    one.seed_mt19937(1, 2)
    refused(L.catan_record_enable(one.h, _ptr(games), 1, 64, _stream()), "MT19937")
    # CATAN_RECORD_AT_DEAL without auto_reset, an unknown mode, slots out of range
    plain.enable_recording(GAMES, capacity=64)
    refused(L.catan_record_arm(plain.h, None, 0, record.RECORD_AT_DEAL, _stream()), "auto_reset")
    refused(L.catan_record_arm(plain.h, None, 0, 2, _stream()), "mode")
    refused(L.catan_record_arm(plain.h, slots.ctypes.data_as(C.c_void_p), 0, record.RECORD_NOW, _stream()), "k must be")
    refused(L.catan_record_arm(plain.h, slots.ctypes.data_as(C.c_void_p), 17, record.RECORD_NOW, _stream()), "k must be")
    refused(L.catan_record_arm(plain.h, np.array([0, 16], dtype=np.int32).ctypes.data_as(C.c_void_p), 2, record.RECORD_NOW, _stream()), "outside [0, m)")
    refused(L.catan_record_read(plain.h, 16, None, None, None, hp, _stream()), "outside [0, m)")
    refused(L.catan_record_read(plain.h, 0, None, None, None, hp, _stream()), "neither SEALED nor RECORDING")     # an IDLE slot
    assert (_status(plain)[:, 0] == record.IDLE).all()
    # an open deferred sequence: enable, arm, status and read
    env.enable_recording(GAMES, capacity=64)
    env.arm_recording(at_deal=True)
    env.step_deferred(env.sample_scripted_actions(), window=WINDOW)
    refused(L.catan_record_enable(env.h, _ptr(games), 16, 64, _stream()), "deferred step sequence is open")
    refused(L.catan_record_arm(env.h, None, 0, record.RECORD_NOW, _stream()), "deferred step sequence is open")
    refused(L.catan_record_status(env.h, sp, _stream()), "deferred step sequence is open")
    refused(L.catan_record_read(env.h, 0, None, None, None, hp, _stream()), "deferred step sequence is open")
    env.step_flush()
    # the library's own deferred rollout while a slot is armed, in both of its forms
    for fused in (True, False):
        env.set_deferred_fused(fused)
        refused(L.catan_random_rollout_deferred(env.h, 8, WINDOW, _stream()), "is armed")
    env.enable_recording([])                                                                   # off again: the rollout runs
    env.random_rollout_deferred(8, WINDOW)
    with pytest.raises(CatanHipError):
        env.recordings()
    # the lock-step random rollout records: it goes through the same step
    plain.arm_recording()
    plain.random_rollout(0, 20)
    st = _status(plain)
    assert (st[:, 0] == record.RECORDING).all() and (st[:, 2] == 20).all()
    rec = plain.recordings(slots=[3], sealed_only=False)[0]
    final, _, _, rejected = rr.replay_on_cpu(rec.seed, rec.game_id, rec.start_blob, rec.actions, **rec.cfg)
    assert not rejected.any() and np.array_equal(final, plain.export_state([GAMES[3]])[0].cpu().numpy())


def test_a_refused_enable_drops_the_old_slots_and_the_next_enable_works(hip_lib):
    """catan_record_enable has dropped the old slots before it builds the new ones: after an enable the device refuses (a game listed
    twice) recording is off, not back at the earlier slots, and a valid enable of two slots then records as any other"""
    from settlers_of_catan_rl_amd.env import _ptr, _stream
    L = hip_lib
    env = _env(False)
    env.enable_recording(GAMES, capacity=64)
    assert _status(env).shape[0] == len(GAMES)
    twice = torch.tensor([3, 4, 3], dtype=torch.int32, device=env.device)
    assert L.catan_record_enable(env.h, _ptr(twice), 3, 64, _stream()) == EINVAL and b"list a game twice" in L.catan_last_error()
    sp = np.zeros((16, 4), dtype=np.uint32).ctypes.data_as(C.c_void_p)
    assert L.catan_record_status(env.h, sp, _stream()) == EINVAL and b"not enabled" in L.catan_last_error()
    env.enable_recording([31, 32], capacity=8)
    env.arm_recording()
    start = env.export_state([31, 32]).cpu().numpy()
    rows = []
    for _ in range(3):
        a = env.sample_scripted_actions()
        rows.append(a[[31, 32]].cpu().numpy())
        env.step(a)
    st = _status(env)
    assert st.shape == (2, 4) and (st[:, 0] == record.RECORDING).all() and st[:, 1].tolist() == [31, 32] and (st[:, 2] == 3).all(), st
    for s, rec in enumerate(env.recordings(sealed_only=False)):
        assert np.array_equal(rec.start_blob, start[s]) and np.array_equal(rec.actions, np.array([r[s] for r in rows])), s


def _product_replay_reaches_the_final_blob(rec):
    """record.replay: product code only, a one-game VecCatanEnv on the device"""
    steps = list(record.replay(rec))
    assert len(steps) == rec.length and steps[-1][4] and not any(s[4] for s in steps[:-1])
    assert np.array_equal(steps[-1][5], rec.final_blob), rec.game_id


def test_evaluation_records(hip_lib):
    """(i) run_evaluation_episodes(record=4) returns games 0..3 whole; record=None returns the parent's dict key for key"""
    import random
    from settlers_of_catan_rl_amd import evaluation as ev
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy
    n = 16

    def run(**kw):
        env = VecCatanEnv(n, seed=SEED, env_id0=100, auto_reset=False)
        bot = ScriptedPolicy(env)
        return env, ev.run_evaluation_episodes(env, [bot, bot, bot, bot], ev.sample_orders(n, random.Random(2)), max_steps=2500, **kw)
    _, plain = run()
    assert list(plain) == ["winner", "victory_points", "game_steps", "policy_decisions"]
    _, with_stats = run(stats=True, record=None)
    assert list(with_stats) == list(plain) + ["entropy", "value", "action_types", "type_log_probs"]
    env, res = run(record=4)
    assert list(res) == list(plain) + ["records"] and all(np.array_equal(res[k], plain[k]) for k in plain)
    assert len(res["records"]) == 4
    final = env.export_state().cpu().numpy()
    for g, rec in enumerate(res["records"]):
        assert (rec.seed, rec.game_id, rec.length) == (SEED, 100 + g, int(res["game_steps"][g])) and not rec.from_deal and not rec.truncated
        assert np.array_equal(rec.final_blob, final[g])
        _replay_checks(rec)
    _product_replay_reaches_the_final_blob(res["records"][0])
    lines = record.describe(res["records"][1])
    assert len(lines) == res["records"][1].length + 1 and lines[-1].endswith("wins") and any(" dice " in ln for ln in lines)
    with pytest.raises(Exception):
        env.recordings()                                         # the evaluator switched the recorder off again


class _StubTrainer(object):
    def __init__(self, net):
        self.optimiser = torch.optim.Adam(net.parameters(), lr=3e-4)
        self.cfg = type("Cfg", (), {"entropy_coef": 0.0})()

    def update(self, st):
        return (0.0, 0.0, 0.0)


@pytest.mark.parametrize("fused", [True, False])
def test_collector_records(hip_lib, fused):
    """(i) RolloutCollector(record_games=4) under TrainingLoop.run_update, the bot in every seat, on the device loop (_gather_device,
    default deferred window) and on the tensor-operation loop (_gather_tensor): both updates hand back sealed records, each from a deal,
    each replays; the slots are armed again behind every read."""
    from settlers_of_catan_rl_amd import train_loop as tl
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    from settlers_of_catan_rl_amd.rollout import RolloutCollector
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy
    n, T = 16, 400
    env = VecCatanEnv(n, seed=SEED + 1)
    bot = ScriptedPolicy(env)
    col = RolloutCollector(env, bot, T, opponents=[bot], seed=3, record_games=4)
    col.fused_bookkeeping = fused
    net = torch.nn.Linear(3, 3)
    loop = tl.TrainingLoop(env, net, col, _StubTrainer(net), tl.TrainArgs(num_steps=T, total_env_steps=T * n * 50))
    seen = []
    for u in range(2):
        out = loop.run_update()
        recs = out["records"]
        print(f"update {u}: {len(recs)} sealed records, lengths {[r.length for r in recs]}")
        assert len(recs) >= 1
        for rec in recs:
            assert rec.from_deal and not rec.truncated and 0 <= rec.game_id < 4 and rec.cfg["auto_reset"]
            _replay_checks(rec)
        seen.append(recs)
        st = _status(env)
        assert set(st[:, 0].tolist()) <= {record.WAIT_DEAL, record.RECORDING}      # every sealed slot was armed again
    assert all(a.start_blob.tobytes() != b.start_blob.tobytes() for a in seen[0] for b in seen[1])
    _product_replay_reaches_the_final_blob(seen[1][0])
    assert env.invalid_action_count() == 0
