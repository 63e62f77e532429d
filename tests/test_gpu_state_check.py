"""GPU: k_state_check / catan_state_check (csrc/catan_hooks.hip) against the numpy restatement of the rules
(tests/state_check_reference.py), whole violation words; the check=True options of import_state and set_start_pool; check_states on
live games; and the hand-written position played in lock step with the oracle.  Every input is read only: no test hands the engine a
blob that breaks a rule."""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded
import state_check_cases as cases
import state_check_reference as ref
from oracle_vec_env import OracleVecEnv
from settlers_of_catan_rl_amd import position, spec

pytestmark = pytest.mark.gpu
EINVAL = -1
F = spec.state_field


@pytest.fixture(scope="module")
def mixed(oracle):
    """the 512 legal blobs with a planted corruption behind every 16th: (blobs, the reference's masks)"""
    legal, planted = cases.legal_pool(), cases.planted()
    rows, k = [], 0
    for i, b in enumerate(legal):
        rows.append(b)
        if i % 16 == 0 and k < len(planted):
            rows.append(planted[k][1])
            k += 1
    assert k == len(planted)
    blobs = np.array(rows, dtype=np.int32)
    blobs.setflags(write=False)
    return blobs, ref.state_check(blobs)


def _raw_check(hip_lib, blobs, n_bad=None, margin=16):
    """catan_state_check itself on blobs [cnt, 736], viol between sentinel margins -> uint64 numpy [cnt]"""
    bt = torch.from_numpy(np.array(np.asarray(blobs).T, order="C")).cuda()
    cnt = bt.shape[1]
    whole, viol = guarded.sentinel_output(cnt, torch.int64, margin, lead=margin, sentinel=guarded.SENTINEL32)
    rc = hip_lib.catan_state_check(guarded.ptr(bt), cnt, guarded.ptr(viol), guarded.ptr(n_bad), guarded.stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert guarded.intact(whole, viol)
    return viol.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("cnt", [1, 63, 64, 65, 257, None])
def test_viol_equals_the_reference_at_every_wave_edge(hip_lib, mixed, cnt):
    blobs, want = mixed
    if cnt is not None:                                       # a window that starts on a planted blob (row 1), another one per cnt
        blobs, want = blobs[1 + cnt:1 + 2 * cnt] if cnt > 1 else blobs[1:2], want[1 + cnt:1 + 2 * cnt] if cnt > 1 else want[1:2]
        assert cnt == 1 or (want != 0).any()
    assert (want != 0).any() and hip_lib.catan_state_check_rules() == len(spec.STATE_CHECK_RULES)
    n_bad = torch.zeros(1, dtype=torch.int64, device="cuda")
    got = _raw_check(hip_lib, blobs, n_bad)
    miss = np.flatnonzero(got != want)
    assert len(miss) == 0, [(int(i), ref.explain(got[i]), ref.explain(want[i])) for i in miss[:6]]
    assert int(n_bad.item()) == int((want != 0).sum())
    _raw_check(hip_lib, blobs, n_bad)
    assert int(n_bad.item()) == 2 * int((want != 0).sum())     # added to, not stored


def test_every_planted_corruption_gives_its_whole_mask(hip_lib, oracle):
    planted = cases.planted()
    got = _raw_check(hip_lib, np.array([b for _, b, _ in planted]))
    for (name, _, rules), g in zip(planted, got):
        assert int(g) == cases.expected_mask(rules), (name, ref.explain(g), sorted(rules))


def test_total_on_every_single_word_corruption(hip_lib, oracle):
    """one legal blob, each of its 736 words in turn at each of -1, 255, 256, 2^31 - 1, -2^31: 3 680 blobs in one launch, read only"""
    blobs = cases.totality_blobs()
    got, want = _raw_check(hip_lib, blobs), ref.state_check(blobs)
    miss = np.flatnonzero(got != want)
    assert len(miss) == 0, [(int(i) // 5, cases.TOTALITY_VALUES[int(i) % 5], ref.explain(got[i]), ref.explain(want[i])) for i in miss[:6]]
    assert (want != 0).sum() > 2000


def test_refusals_launch_nothing_and_the_python_forms_agree(hip_lib, mixed):
    blobs, want = mixed
    bt = torch.from_numpy(np.ascontiguousarray(blobs[:64].T)).cuda()
    whole, viol = guarded.sentinel_output(64, torch.int64, 16, lead=16, sentinel=guarded.SENTINEL32)
    n_bad = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    for args in ((None, 64, guarded.ptr(viol)), (guarded.ptr(bt), 64, None), (guarded.ptr(bt), 0, guarded.ptr(viol)), (guarded.ptr(bt), -3, guarded.ptr(viol))):
        assert hip_lib.catan_state_check(args[0], args[1], args[2], guarded.ptr(n_bad), guarded.stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool((whole.view(torch.int32) == guarded.SENTINEL32).all()) and int(n_bad.item()) == 7
    assert hip_lib.catan_state_check(guarded.ptr(bt), 64, guarded.ptr(viol), None, guarded.stream()) == 0      # n_bad may be NULL
    torch.cuda.synchronize()
    assert guarded.intact(whole, viol) and np.array_equal(viol.cpu().numpy().view(np.uint64), want[:64])
    got = position.check_blobs(blobs[:100])
    assert got.dtype == torch.uint64 and got.is_cuda and np.array_equal(got.cpu().numpy(), want[:100])
    assert np.array_equal(position.check_blobs(torch.from_numpy(blobs[1].copy())).cpu().numpy(), want[1:2])
    with pytest.raises(ValueError):
        position.check_blobs(blobs[:3].T)


def _env(n=64, **kw):
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    return VecCatanEnv(n, seed=3, env_id0=5, **kw)


def _snapshot(env):
    return env.export_state().clone(), env.get_action_masks_packed().clone()


def test_import_state_check_refuses_a_bad_blob_and_changes_nothing(hip_lib, mixed):
    legal = cases.legal_pool()[100:164].copy()
    bad = legal.copy()
    bad[17] = cases.planted()[12][1]
    name, _, rules = cases.planted()[12]
    env = _env()
    env.random_rollout(0, 40)
    before = _snapshot(env)
    with pytest.raises(ValueError) as e:
        env.import_state(bad, check=True)
    assert "blob 17" in str(e.value) and all(r in str(e.value) for r in rules) and "1 of 64" in str(e.value)
    after = _snapshot(env)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert np.array_equal(env.check_blobs(bad).cpu().numpy(), ref.state_check(bad))
    # good blobs: exactly what check=False does
    twin = _env()
    twin.random_rollout(0, 40)
    env.import_state(legal, check=True)
    twin.import_state(legal)
    a, b = _snapshot(env), _snapshot(twin)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], before[0])
    # nine bad blobs: the first eight are named
    many = legal.copy()
    many[10:19] = cases.planted()[12][1]
    with pytest.raises(ValueError) as e:
        env.import_state(many, [int(g) for g in range(64)], check=True)
    assert "9 of 64" in str(e.value) and "blob 17" in str(e.value) and "blob 18" not in str(e.value) and "1 more" in str(e.value)


def test_set_start_pool_check_refuses_a_bad_blob_and_keeps_the_pool(hip_lib, mixed):
    legal = cases.legal_pool()
    live = legal[(F(legal, "winner")[:, 0] == 0)][:64]
    other = legal[(F(legal, "winner")[:, 0] == 0)][64:128]
    bad = other.copy()
    bad[40] = cases.planted()[13][1]
    env, twin = _env(), _env()
    for e in (env, twin):
        e.set_start_pool(live, check=(e is env))
    with pytest.raises(ValueError) as err:
        env.set_start_pool(bad, check=True)
    assert "blob 40" in str(err.value) and "set_start_pool" in str(err.value)
    for e in (env, twin):
        e.reset()
    a, b = _snapshot(env), _snapshot(twin)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ca, cb = env.start_pool_counts(), twin.start_pool_counts()
    assert ca["pool"] == cb["pool"] == 64 and np.array_equal(ca["per_entry"], cb["per_entry"]) and len(ca["per_entry"]) == 64


def test_check_states_is_all_zero_on_live_games(hip_lib):
    env = _env(96)
    assert not env.check_states().cpu().numpy().any()
    step = 0
    for chunk in (300, 700, 1000, 2000):
        env.random_rollout(step, chunk)
        step += chunk
        v = env.check_states().cpu().numpy()
        assert not v.any(), (step, position.describe_bad(v))
    assert step == 4000
    assert not env.check_states([0, 95, 31]).cpu().numpy().any() and env.check_states([0, 95, 31]).shape == (3,)
    env.random_rollout_deferred(400, 8)
    v = env.check_states().cpu().numpy()
    assert not v.any(), position.describe_bad(v)


def test_the_written_position_plays_like_the_oracles(hip_lib, oracle):
    p = cases.written_position()
    blob = p.to_blob()
    n = 4
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    env, twin = VecCatanEnv(n, seed=9, env_id0=2), OracleVecEnv(n, seed=9, env_id0=2)
    env.import_state(np.repeat(blob[None], n, 0), check=True)
    twin.import_state(np.repeat(blob[None], n, 0))
    assert np.array_equal(env.get_action_masks().cpu().numpy(), twin.get_action_masks().numpy())
    got = position.Position.from_env(env, 2)
    assert np.array_equal(got.to_blob(), blob)
    q = position.Position.from_blob(blob)
    q["cur_longest_path"][:] = 0
    assert list(q.refresh(env)["cur_longest_path"]) == [1, 1, 1, 1]          # the device's own search, on an env of its own
    assert np.array_equal(env.export_state().cpu().numpy(), np.repeat(blob[None], n, 0))
    for t in range(200):
        a = env.sample_random_actions(t)
        reward, done = env.step(a)
        r_h, d_h = reward.cpu().numpy().copy(), done.cpu().numpy().copy()
        tr, td = twin.step(a.cpu())
        assert np.array_equal(r_h, tr.numpy()) and np.array_equal(d_h, td.numpy()), t
        got, want = env.export_state().cpu().numpy(), twin.export_state().numpy()
        for g in range(n):
            assert np.array_equal(got[g], want[g]), (t, g, spec.describe_state_diff(got[g], want[g]))
        assert np.array_equal(env.get_action_masks().cpu().numpy(), twin.get_action_masks().numpy()), t
    assert not env.check_states().cpu().numpy().any()
