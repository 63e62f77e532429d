"""CPU checks of the PPO update diagnostics (ppo.ppo_diag / ppo.diag_summary, PPOConfig.diagnostics / target_kl):
the numpy helper against words written out by hand, the package's torch form against the helper, the summary's arithmetic, what the
trainer calls and when, the reduction over ranks (gloo, two shards of one rollout), and where the read-out surfaces.  The kernel itself
is compared with the same helper in tests/test_gpu_ppo_diag.py."""
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import ppo_diag_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 6
N_GAMES = 10


# ---------------------------------------------------------------------------------------------- the helper, by hand
def test_helper_on_four_rows_written_out_by_hand():
    """clip 0.2, no normaliser.  Row A: inside the clip (d = 0), value inside.  Row B: outside upwards (d = 0.5, ratio 1.65) with
    adv = 2 > 0: s1 = 3.30 > s2 = 2.4, the policy gradient is zeroed.  Row C: outside downwards (d = -0.5, ratio 0.61) with adv = 1 > 0:
    s1 = 0.61 < s2 = 0.8, the gradient stays.  Row D: inside (d = 0), value-clipped (v - vp = 0.5) with l1 = (1 - 1)^2 = 0 <
    l2 = (0.7 - 1)^2: the value gradient is zeroed."""
    logp = [-1.0, -0.5, -1.5, -2.0]
    old = [-1.0, -1.0, -1.0, -2.0]
    adv = [1.0, 2.0, 1.0, -1.0]
    v = [0.5, 0.0, 1.0, 1.0]
    vp = [0.5, 0.0, 1.0, 0.5]
    ret = [1.0, 0.0, 0.0, 1.0]
    w, a = R.reference_words(logp, old, adv, v, vp, ret, 0.2, None, entropy=1.5, grad_norm=0.75, max_grad_norm=0.5)
    k3 = math.expm1(0.5) - 0.5 + math.expm1(-0.5) + 0.5
    hand = [4, 1,                       # rows, steps
            0.0, k3, 0.5, 0.5,          # sum(-d), sum(expm1(d) - d), max d, max -d
            2, 1, 1, 1,                 # outside (B, C); policy gradient zeroed (B); |v - vp| > clip (D); value gradient zeroed (D)
            2.0, 2.0,                   # ret = 1, 0, 0, 1
            -0.5, 1.25,                 # e = ret - v = 0.5, 0, -1, 0
            0.0, 1.5,                   # e0 = ret - vp = 0.5, 0, -1, 0.5
            1.5, 0.75, 1, 0.75]         # entropy, gradient norm, norm > 0.5, max norm
    assert len(hand) == R.WORDS
    for i, (x, y) in enumerate(zip(w, hand)):
        assert abs(x - y) <= 1e-15, (i, x, y)
    assert a[2] == 1.0 and a[12] == 1.5 and a[14] == 2.0
    # no scalars: their words stay zero; max_grad_norm <= 0 never counts a clipped step
    w2, _ = R.reference_words(logp, old, adv, v, vp, ret, 0.2, None)
    assert list(w2[16:]) == [0, 0, 0, 0] and list(w2[:16]) == list(w[:16])
    assert R.reference_words(logp, old, adv, v, vp, ret, 0.2, None, grad_norm=0.75, max_grad_norm=0.0)[0][18] == 0
    # the normaliser: vp, ret given denormalised; (x - 150) / 150.0001 brings the same rows back to within 1e-6, the counts stay
    den = float(np.float32(150.0)) + 1e-4
    w3, _ = R.reference_words(logp, old, adv, v, [150 + den * x for x in vp], [150 + den * x for x in ret], 0.2, (150.0, 150.0))
    assert list(w3[6:10]) == [2, 1, 1, 1] and abs(w3[13] - 1.25) < 1e-4 and abs(w3[15] - 1.5) < 1e-4


def test_builder_replaces_few_rows_in_every_case():
    for B, seed in R.CASES:
        for clip, norm in R.SETTINGS:
            x = R.build_inputs(B, seed, clip, norm)          # (asserts <= 2 % itself)
            assert x["replaced"] <= 0.02 * B and all(x[k].dtype == np.float32 and x[k].shape == (B,) for k in ("logp", "old_logp", "adv", "v", "vp", "ret"))
            if B > 1000:                                     # every decision has rows on both sides
                w, _ = R.reference_words(x["logp"], x["old_logp"], x["adv"], x["v"], x["vp"], x["ret"], clip, norm)
                assert 0 < w[7] < w[6] < B and 0 < w[9] < w[8] < B


# ---------------------------------------------------------------------------------------------- the package's torch form
def _torch_block(x, clip, norm, block=None, **kw):
    from settlers_of_catan_rl_amd import ppo
    block = torch.zeros(20, dtype=torch.float64) if block is None else block
    t = {k: torch.from_numpy(x[k]) for k in ("logp", "v", "old_logp", "adv", "vp", "ret")}
    ppo.ppo_diag(block, t["logp"], t["v"], t["old_logp"], t["adv"], t["vp"], t["ret"], clip, norm, **kw)
    return block


@pytest.mark.parametrize("B,seed", R.CASES)
def test_torch_form_equals_the_helper(B, seed):
    for clip, norm in R.SETTINGS:
        x = R.build_inputs(B, seed, clip, norm)
        ref, a = R.reference_words(x["logp"], x["old_logp"], x["adv"], x["v"], x["vp"], x["ret"], clip, norm)
        got = _torch_block(x, clip, norm)
        R.assert_words(got.numpy(), ref, a)
        assert list(got[16:].numpy()) == [0, 0, 0, 0]
        # with the scalars, and a second call into the same block
        ent, gn = torch.tensor(1.25, dtype=torch.float32), torch.tensor([0.625], dtype=torch.float32)
        filled = torch.full((20,), 3.0, dtype=torch.float64)
        _torch_block(x, clip, norm, block=filled)
        assert list(filled[16:].numpy()) == [3, 3, 3, 3]                       # no scalar: the words are left as they were
        two = _torch_block(x, clip, norm, block=got, entropy=ent, grad_norm=gn, max_grad_norm=0.5)
        ref2 = R.combine([(ref, a), R.reference_words(x["logp"], x["old_logp"], x["adv"], x["v"], x["vp"], x["ret"], clip, norm, entropy=1.25,
                                                      grad_norm=0.625, max_grad_norm=0.5)])
        R.assert_words(two.numpy(), *ref2)
        assert two[18] == 1 and two[19] == 0.625 and two[1] == 2


def test_block_is_checked():
    from settlers_of_catan_rl_amd import ppo
    x = {k: torch.zeros(3) for k in "abcdef"}
    with pytest.raises(ValueError):
        ppo.ppo_diag(torch.zeros(19, dtype=torch.float64), *x.values(), 0.2, None)
    with pytest.raises(ValueError):
        ppo.ppo_diag(torch.zeros(20, dtype=torch.float32), *x.values(), 0.2, None)


# ---------------------------------------------------------------------------------------------- diag_summary
def test_diag_summary_on_hand_made_blocks():
    from settlers_of_catan_rl_amd import ppo
    b = np.zeros((2, 20))
    #        rows steps  k1   k3   up   down out  pz  vout vz   Sret Sret2  Se  Se2  Se0 Se02  ent  gn  clipped gmax
    b[0] = [100, 4, 0.5, 0.25, 0.3, 0.2, 10, 5, 20, 8, 50, 125, 10, 26, 20, 54, 6.0, 2.0, 1, 0.75]
    b[1] = [300, 4, 3.0, 1.50, 0.1, 0.6, 90, 30, 60, 12, 0, 300, 30, 78, 0, 300, 4.0, 6.0, 3, 2.5]
    s = ppo.diag_summary(b)
    assert s["rows"] == [100, 300] and s["steps"] == [4, 4]
    assert s["approx_kl"] == [0.0025, 0.005] and s["approx_kl_k1"] == [0.005, 0.01]
    assert s["max_log_ratio_up"] == [0.3, 0.1] and s["max_log_ratio_down"] == [0.2, 0.6]
    assert s["clip_fraction"] == [0.1, 0.3] and s["policy_grad_zero_fraction"] == [0.05, 0.1]
    assert s["value_clip_fraction"] == [0.2, 0.2] and s["value_grad_zero_fraction"] == [0.08, 0.04]
    # epoch 0: Var(ret) = 1.25 - 0.25 = 1, Var(e) = 0.26 - 0.01 = 0.25, Var(e0) = 0.54 - 0.04 = 0.5; epoch 1: Var(ret) = 1, Var(e) = 0.26 - 0.01, Var(e0) = 1
    assert np.allclose(s["explained_variance"], [0.75, 0.75], rtol=0, atol=1e-12) and np.allclose(s["explained_variance_old"], [0.5, 0.0], rtol=0, atol=1e-12)
    assert s["entropy"] == [1.5, 1.0] and s["grad_norm_mean"] == [0.5, 1.5] and s["grad_norm_max"] == [0.75, 2.5] and s["grad_clipped_fraction"] == [0.25, 0.75]
    u = s["update"]
    assert u["rows"] == 400 and u["steps"] == 8 and u["approx_kl"] == 1.75 / 400 and u["approx_kl_k1"] == 3.5 / 400
    assert u["max_log_ratio_up"] == 0.3 and u["max_log_ratio_down"] == 0.6 and u["grad_norm_max"] == 2.5
    assert u["clip_fraction"] == 0.25 and u["policy_grad_zero_fraction"] == 35 / 400 and u["value_clip_fraction"] == 0.2 and u["value_grad_zero_fraction"] == 0.05
    var_ret = 425 / 400 - (50 / 400) ** 2
    assert abs(u["explained_variance"] - (1 - (104 / 400 - 0.01) / var_ret)) < 1e-12
    assert abs(u["explained_variance_old"] - (1 - (354 / 400 - 0.0025) / var_ret)) < 1e-12
    assert u["entropy"] == 1.25 and u["grad_norm_mean"] == 1.0 and u["grad_clipped_fraction"] == 0.5
    assert set(s) == {"approx_kl", "approx_kl_k1", "max_log_ratio_up", "max_log_ratio_down", "clip_fraction", "policy_grad_zero_fraction",
                      "value_clip_fraction", "value_grad_zero_fraction", "explained_variance", "explained_variance_old", "entropy",
                      "grad_norm_mean", "grad_norm_max", "grad_clipped_fraction", "rows", "steps", "update"}
    assert set(u) == set(s) - {"update"}
    # constant returns: Var(ret) = 0 -> NaN, not a division by zero
    c = np.zeros((1, 20)); c[0, :2] = (10, 1); c[0, 10:12] = (20, 40); c[0, 12:14] = (1, 3)
    z = ppo.diag_summary(c)
    assert math.isnan(z["explained_variance"][0]) and math.isnan(z["explained_variance_old"][0]) and math.isnan(z["update"]["explained_variance"])
    assert z["approx_kl"] == [0.0] and z["clip_fraction"] == [0.0]
    with pytest.raises(ValueError):
        ppo.diag_summary(np.zeros((2, 19)))


# ---------------------------------------------------------------------------------------------- the trainer on CPU
# the torch stand-ins of the HIP back-ends and the rollout of tests/test_multi_rank_learner_cpu.py (copied: that module is not imported)
def _install_cpu_backends():
    from settlers_of_catan_rl_amd import ppo

    def gae_raw(r, v, m, gamma, lam):
        Tn = r.shape[0]
        ret = torch.zeros_like(r)
        gae = torch.zeros_like(r[0])
        for t in reversed(range(Tn)):
            delta = r[t] + gamma * v[t + 1] * m[t + 1] - v[t]
            gae = delta + gamma * lam * m[t + 1] * gae
            ret[t] = gae + v[t]
        adv = ret - v[:-1]
        a = adv.double()
        return ret, adv, torch.stack((a.sum(), (a * a).sum(), torch.tensor(float(a.numel()), dtype=torch.float64)))

    def adv_normalise(adv, stats):
        cnt, mean = stats[2], stats[0] / stats[2]
        std = torch.sqrt((stats[1] - cnt * mean * mean) / (cnt - 1))
        return ((adv.double() - mean) / (std + 1e-5)).float()

    def loss(lp, v, old_lp, adv, v_old, ret, clip, value_coef, norm):
        lp, v, old_lp, adv, v_old, ret = (x.reshape(-1) for x in (lp, v, old_lp, adv, v_old, ret))
        if norm is not None:
            v_old, ret = (v_old - norm[0]) / (norm[1] + 1e-4), (ret - norm[0]) / (norm[1] + 1e-4)
        ratio = torch.exp(lp - old_lp)
        al = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv).mean()
        vc = v_old + (v - v_old).clamp(-clip, clip)
        vl = 0.5 * torch.max((v - ret).pow(2), (vc - ret).pow(2)).mean()
        return vl * value_coef + al, torch.stack((al.detach(), vl.detach()))
    saved = (ppo._gae_raw, ppo._adv_normalise, ppo._loss_backend)
    ppo._gae_raw, ppo._adv_normalise, ppo._loss_backend = gae_raw, adv_normalise, loss
    return saved


def _make_rollout(n_games, env_id0):
    """a rollout storage filled by the real collector (oracle-backed env, random-initialised net, fixed seeds)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle_vec_env import OracleVecEnv
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    from settlers_of_catan_rl_amd.rollout import RolloutCollector
    torch.manual_seed(7)
    actor = CatanPolicy().eval()
    env = OracleVecEnv(n_games, seed=9, env_id0=env_id0)
    env.advance_random(900)
    col = RolloutCollector(env, actor, T, seed=100 + env_id0)
    st = col.gather_rollouts()
    for (t, g) in ((2, 1), (4, 6), (1, 8)):                # game ends for the learner's benefit: terminal masks + win rewards
        st.masks[t + 1, g] = 0.0
        st.rewards[t, g] = 500.0
    return st


def _slice_storage(st, lo, hi):
    from settlers_of_catan_rl_amd.rollout import RolloutStorage
    out = RolloutStorage(st.T, hi - lo, "cpu")
    for k in ("obs_f", "lists", "lens", "masks", "rewards", "actions", "action_log_probs", "action_masks"):
        setattr(out, k, getattr(st, k)[:, lo:hi].clone())
    return out


@pytest.fixture(scope="module")
def rollout():
    return _make_rollout(N_GAMES, 0)


@pytest.fixture()
def cpu_backends():
    """the stand-ins, and a counter in front of ppo._diag_backend; everything is put back afterwards"""
    from settlers_of_catan_rl_amd import ppo
    saved, diag = _install_cpu_backends(), ppo._diag_backend
    calls = []

    def counting(*a):
        calls.append(a[1].numel())
        return diag(*a)
    ppo._diag_backend = counting
    yield calls
    ppo._gae_raw, ppo._adv_normalise, ppo._loss_backend = saved
    ppo._diag_backend = diag


def _trainer(**cfg):
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    from settlers_of_catan_rl_amd.train import PPOTrainer, PPOConfig
    torch.manual_seed(123)
    return PPOTrainer(CatanPolicy(), PPOConfig(**cfg), autocast_dtype=None, seed=0)


def test_diagnostics_off_calls_nothing(rollout, cpu_backends):
    from settlers_of_catan_rl_amd.train import PPOConfig
    assert PPOConfig.diagnostics is False and PPOConfig.target_kl is None
    tr = _trainer(ppo_epoch=2, num_mini_batch=1)
    assert tr.diagnostics is None
    losses = tr.update(rollout)
    assert cpu_backends == [] and tr.diagnostics is None and len(losses) == 3 and set(tr.timings) == {"values_s", "gae_s", "minibatches_s"}


def test_diagnostics_on_counts_every_step(rollout, cpu_backends):
    tr = _trainer(ppo_epoch=2, num_mini_batch=1, diagnostics=True)
    vl, al, el = tr.update(rollout)
    d = tr.diagnostics
    assert cpu_backends == [T * N_GAMES] * 2
    assert d["rows"] == [T * N_GAMES] * 2 and d["steps"] == [1, 1] and d["update"]["rows"] == 2 * T * N_GAMES and d["update"]["steps"] == 2
    assert abs(d["update"]["entropy"] * tr.cfg.entropy_coef - el) <= 1e-5 * abs(el)
    assert set(tr.timings) == {"values_s", "gae_s", "minibatches_s"}                     # nothing new where bench.py spreads the timings
    u = d["update"]
    for k in ("clip_fraction", "policy_grad_zero_fraction", "value_clip_fraction", "value_grad_zero_fraction", "grad_clipped_fraction"):
        assert 0.0 <= u[k] <= 1.0
    assert u["policy_grad_zero_fraction"] <= u["clip_fraction"] and u["grad_norm_max"] >= u["grad_norm_mean"] > 0
    assert u["approx_kl"] >= 0 and d["approx_kl"][1] > 0            # the second epoch sees a net that has taken a step
    # the same update without diagnostics returns the same losses: the read-out changes nothing
    tr2 = _trainer(ppo_epoch=2, num_mini_batch=1)
    assert tr2.update(rollout) == (vl, al, el)


def test_target_kl_stops_after_the_first_epoch(rollout, cpu_backends):
    """target_kl = 0: the first epoch's second minibatch sees a net that has taken one step, so its KL is above zero and the other two
    epochs are skipped; the losses average over the two steps taken."""
    tr = _trainer(ppo_epoch=3, num_mini_batch=2, diagnostics=True, target_kl=0.0)
    vl, al, el = tr.update(rollout)
    d = tr.diagnostics
    assert len(cpu_backends) == 2 and d["steps"] == [2] and d["rows"] == [T * N_GAMES] and d["approx_kl"][0] > 0.0
    assert abs(d["update"]["entropy"] * tr.cfg.entropy_coef - el) <= 1e-5 * abs(el)     # the mean over the steps taken, not over 3 epochs
    # a generous target never stops early
    del cpu_backends[:]
    tr = _trainer(ppo_epoch=3, num_mini_batch=2, diagnostics=True, target_kl=1e9)
    tr.update(rollout)
    assert len(cpu_backends) == 6 and tr.diagnostics["steps"] == [2, 2, 2]


def test_target_kl_needs_diagnostics():
    with pytest.raises(ValueError):
        _trainer(target_kl=0.01)
    tr = _trainer()
    tr.cfg.target_kl = 0.01            # (set behind the constructor's back: update() refuses too, before it touches the rollout)
    with pytest.raises(ValueError):
        tr.update(None)


# ---------------------------------------------------------------------------------------------- two ranks
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


class _RowwisePolicy(torch.nn.Module):
    """What PPOTrainer needs of a policy, with a forward that gives a row the same bits whatever batch it sits in: computed per row in
    fp64 and rounded to fp32 once (the real net's fp32 GEMMs, and even torch's vectorised fp32 softplus with its scalar tail, round a row
    differently in a 30-row and in a 60-row batch: by ~1e-7 of a log-prob and so by ~1e-5 of an epoch's approx_kl - measured - which
    would hide a wrong reduction behind forward noise).  One Bernoulli "head" on the action type's parity, a linear value head."""
    VALUE_MEAN, VALUE_STD = 0.0, 1.0

    def __init__(self, width):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.wa = torch.nn.Parameter(0.02 * torch.randn(width, generator=g))
        self.wv = torch.nn.Parameter(0.02 * torch.randn(width, generator=g))

    def denormalise(self, x):
        return x * self.VALUE_STD + self.VALUE_MEAN

    def get_value(self, f, lists, lens):
        return (f.double() * self.wv.double()).sum(-1).float()[:, None]

    def evaluate_actions(self, f, lists, lens, masks, acts):
        z = (f.double() * self.wa.double()).sum(-1)
        sign = (acts[:, 0] % 2).to(z.dtype) * 2.0 - 1.0
        lp = (-torch.nn.functional.softplus(-sign * z)).float()
        ent = (torch.nn.functional.softplus(z) - z * torch.sigmoid(z)).float().mean()
        return self.get_value(f, lists, lens), lp[:, None], ent


def _train_with_diagnostics(st):
    """one epoch of one minibatch: the step's rows are evaluated with the SAME parameters on one process and on two ranks (after a step
    the parameters of the two runs differ by the 1e-5 of the shard test, and with them every later row)"""
    from settlers_of_catan_rl_amd.train import PPOTrainer, PPOConfig
    from settlers_of_catan_rl_amd import dist as cdist
    net = _RowwisePolicy(st.obs_f.shape[-1])
    cdist.broadcast_parameters(net)
    tr = PPOTrainer(net, PPOConfig(ppo_epoch=1, num_mini_batch=1, diagnostics=True), autocast_dtype=None, seed=0)
    tr.update(st)
    return tr.diagnostics


def _worker(rank, world, n_per, port, path, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    torch.set_num_threads(2)
    from settlers_of_catan_rl_amd import dist as cdist
    _install_cpu_backends()
    cdist.init_from_env(backend="gloo")
    full = torch.load(path, weights_only=False)
    q.put((rank, _train_with_diagnostics(_slice_storage(full, rank * n_per, (rank + 1) * n_per))))
    cdist.finalize()


def test_two_ranks_give_the_single_process_summary(rollout, cpu_backends, tmp_path):
    """Two gloo ranks on the two halves of the rollout against one process on all of it (one minibatch = the whole shard, so the two
    ranks' step is the single process's step; _RowwisePolicy keeps a row's log-prob and value the same bits in both): rows, steps and
    the counts behind every fraction exactly, everything built from the fp64 row sums within 1e-9 relative, the gradient norms within
    the 1e-5 the shard test of the parameters uses.  The entropy is not a row sum: every rank hands in the fp32 mean over its own rows,
    and the mean of two fp32 means of 30 rows differs from the fp32 mean of 60 rows by rounding - a few 2^-24; 1e-6 relative."""
    path = str(tmp_path / "rollout.pt")
    torch.save(rollout, path)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, N_GAMES // 2, port, path, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=600) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    one = _train_with_diagnostics(rollout)
    for a, b in ((got[0], got[1]), (got[0]["update"], got[1]["update"])):                  # every rank holds the global summary
        assert all(_same(a[k], b[k], 0.0) for k in a if k != "update")
    for d, e in ((got[0], one), (got[0]["update"], one["update"])):
        for k in ("rows", "steps", "clip_fraction", "policy_grad_zero_fraction", "value_clip_fraction", "value_grad_zero_fraction", "grad_clipped_fraction"):
            assert d[k] == e[k], (k, d[k], e[k])
        for k in ("approx_kl", "approx_kl_k1", "max_log_ratio_up", "max_log_ratio_down", "explained_variance", "explained_variance_old"):
            assert _same(d[k], e[k], 1e-9), (k, d[k], e[k])
        assert _same(d["entropy"], e["entropy"], 1e-6), (d["entropy"], e["entropy"])
        for k in ("grad_norm_mean", "grad_norm_max"):
            assert _same(d[k], e[k], 1e-5), (k, d[k], e[k])


def _same(a, b, rel):
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and bool(np.all((np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b))) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------------------------------------- where it surfaces
class _Env(object):
    n = 10
    def set_reward_annealing_factor(self, f): pass


class _Storage(object):
    games_complete = 3


class _Collector(object):
    N = 10
    def gather_rollouts(self): return _Storage()
    def after_rollouts(self): pass


class _Trainer(object):
    def __init__(self, net, diagnostics):
        self.optimiser = torch.optim.Adam(net.parameters(), lr=3e-4)
        class Cfg: entropy_coef = 0.0
        self.cfg = Cfg()
        self.diagnostics = diagnostics
    def update(self, st): return (0.1, 0.2, 0.3)


class _OldTrainer(object):             # a trainer from before the feature: no attribute at all
    def __init__(self, net):
        self.optimiser = torch.optim.Adam(net.parameters(), lr=3e-4)
        class Cfg: entropy_coef = 0.0
        self.cfg = Cfg()
    def update(self, st): return (0.1, 0.2, 0.3)


def test_run_update_carries_ppo_only_with_diagnostics():
    from settlers_of_catan_rl_amd import ppo, train_loop as tl
    net = torch.nn.Linear(3, 3)
    args = tl.TrainArgs(num_steps=4, total_env_steps=4 * 10 * 50)
    summary = ppo.diag_summary(np.ones((2, 20)))
    out = tl.TrainingLoop(_Env(), net, _Collector(), _Trainer(net, summary), args).run_update()
    assert out["ppo"] is summary and out["losses"] == (0.1, 0.2, 0.3)
    assert "ppo" not in tl.TrainingLoop(_Env(), net, _Collector(), _Trainer(net, None), args).run_update()
    assert "ppo" not in tl.TrainingLoop(_Env(), net, _Collector(), _OldTrainer(net), args).run_update()
    import json
    json.dumps(out["ppo"])             # tools/train.py prints the update's dict as one JSON line


def test_reference_adapter_accumulates_the_same_way(monkeypatch):
    """reference_api.PPO with args.ppo_diagnostics: same return value and timings, the summary in `.diagnostics`; absent or false: None"""
    import types
    from oracle_vec_env import OracleVecEnv
    from settlers_of_catan_rl_amd import reference_api as ra

    def torch_gae(rewards, values, masks, gamma, lam, **_kw):
        returns = torch.zeros_like(rewards)
        gae = 0
        for step in reversed(range(rewards.shape[0])):
            delta = rewards[step] + gamma * values[step + 1] * masks[step + 1] - values[step]
            gae = delta + gamma * lam * masks[step + 1] * gae
            returns[step] = gae + values[step]
        adv = returns - values[:-1]
        return returns, (adv - adv.mean()) / (adv.std() + 1e-5)

    def torch_loss(lp, v, old_lp, adv, v_old, ret, clip, value_coef, value_normaliser=None):
        lp, v, old_lp, adv, v_old, ret = (x.reshape(-1) for x in (lp, v, old_lp, adv, v_old, ret))
        if value_normaliser is not None:
            m, s = value_normaliser
            v_old, ret = (v_old - m) / (s + 1e-4), (ret - m) / (s + 1e-4)
        ratio = torch.exp(lp - old_lp)
        al = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv).mean()
        vc = v_old + (v - v_old).clamp(-clip, clip)
        vl = 0.5 * torch.max((v - ret).pow(2), (vc - ret).pow(2)).mean()
        return vl * value_coef + al, torch.stack((al.detach(), vl.detach()))
    monkeypatch.setattr(ra, "_GAE", torch_gae)
    monkeypatch.setattr(ra, "_LOSS", torch_loss)
    n, Tn = 6, 7
    mgr = ra.SubProcGameManager([ra.make_game_manager(3, Tn), ra.make_game_manager(3, Tn)], env_factory=lambda k: OracleVecEnv(k, 5),
                                self_play=True, autocast_dtype=None)
    args = types.SimpleNamespace(num_steps=Tn, num_processes=2, num_envs_per_process=3, gamma=0.999, gae_lambda=0.95, lr=3e-4, eps=1e-5,
                                 clip_param=0.2, ppo_epoch=2, num_mini_batch=3, value_loss_coef=1.0, entropy_coef_start=0.04, max_grad_norm=0.5,
                                 truncated_seq_len=10, ppo_diagnostics=True)
    bp = ra.BatchProcessor(args, lstm_dim=256, device="cpu")
    bp.process_rollouts(mgr.gather_rollouts())
    torch.manual_seed(3)
    agent = ra.PPO(ra.build_agent_model("cpu"), args)
    assert agent.diagnostics is None
    vl, al, el = agent.update(bp)
    d = agent.diagnostics
    assert d["rows"] == [3 * (Tn * n // 3)] * 2 and d["steps"] == [3, 3] and set(agent.timings) == {"advantages_s", "minibatches_s"}
    assert abs(d["update"]["entropy"] * agent.entropy_coef - el) <= 1e-5 * abs(el) and d["update"]["grad_norm_max"] > 0
    args.ppo_diagnostics = False
    agent.update(bp)
    assert agent.diagnostics is None
