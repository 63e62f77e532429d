"""Per-row entropy and the log_specific_action_output record of `act`, against what the reference's own net returned from
single-row calls (tests/golden/act_stats.npz, tools/gen_golden_eval_stats.py; inputs and weights of policy_small.npz)."""
import os

import numpy as np
import torch

import policy_fixture as pf
from settlers_of_catan_rl_amd import reference_api

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load():
    g = np.load(os.path.join(GOLD, "policy_small.npz"))
    s = np.load(os.path.join(GOLD, "act_stats.npz"))
    net, _ = pf.load_fixture_policy(g, "ff", "cpu")
    x, B = pf.decode_inputs(g, "ff_")
    return net, x, s


def _rows(x, idx):
    idx = torch.as_tensor(np.asarray(idx, dtype=np.int64))
    return {k: v[idx] for k, v in x.items()}


def _check(net, x, s, prefix, forced=None):
    with torch.no_grad():
        v, a, lp, ent, rec = net.act(x["obs_f"], x["lists"], x["lens"], x["masks"], deterministic=True, condition_on_action_type=forced,
                                     return_entropy=True, return_head_log=True)
    assert torch.equal(a, torch.from_numpy(s[prefix + "actions"].astype(np.int64)))
    assert float((lp[:, 0] - torch.from_numpy(s[prefix + "logp"])).abs().max()) <= 1e-5
    assert ent.shape == (a.shape[0],) and rec.shape == (a.shape[0], 4)
    assert float((ent - torch.from_numpy(s[prefix + "entropy"])).abs().max()) <= 1e-5
    assert float((rec - torch.from_numpy(s[prefix + "log"])).abs().max()) <= 1e-5
    # the default call's outputs are the same
    with torch.no_grad():
        v0, a0, lp0 = net.act(x["obs_f"], x["lists"], x["lens"], x["masks"], deterministic=True, condition_on_action_type=forced)
    assert torch.equal(a0, a) and torch.equal(lp0, lp) and torch.equal(v0, v)
    return ent


def test_torch_path_entropy_and_log_records_match_reference():
    net, x, s = _load()
    g = np.load(os.path.join(GOLD, "policy_small.npz"))
    # the single-row calls (their mask tables restored before each: tools/gen_golden_eval_stats.py) are the batched call
    assert np.abs(s["free_logp"] - g["ff_act_logp"][:, 0]).max() <= 1e-5
    ent = _check(net, x, s, "free_")
    assert float(ent.min()) >= 0.0
    xf = _rows(x, s["forced_rows"])
    _check(net, xf, s, "forced_", torch.from_numpy(s["forced_type"].astype(np.int64)))


def test_reference_api_act_returns_reference_entropy_and_log_tuples():
    net, x, s = _load()
    pol = reference_api.SettlersAgentPolicy(net, autocast_dtype=None)
    rows = list(range(0, 320, 23))
    for i in rows:
        obs = reference_api.obs_flat_to_dict(x["obs_f"][i:i + 1], x["lists"][i:i + 1])
        masks = reference_api.masks_flat_to_list(x["masks"][i:i + 1])
        with torch.no_grad():
            out = pol.act(obs, None, None, masks, deterministic=True, return_entropy=True, log_specific_action_output=True)
        assert len(out) == 6
        value, actions, lp, hidden, entropy, log = out
        assert torch.is_tensor(entropy) and entropy.dim() == 0
        assert abs(float(entropy) - float(s["free_entropy"][i])) <= 1e-5
        typ = int(s["free_actions"][i, 0])
        rec, head = s["free_log"][i], int(s["free_log_head"][i])
        assert log[0][0] is None and log[0][1] == 0 and log[0][3] == int(rec[1]) and log[0][4] == typ
        assert abs(float(log[0][2]) - float(rec[0])) <= 1e-5
        if head < 0:
            assert len(log) == 1
        else:
            assert len(log) == 2
            t, h, p, n, act = log[1]
            assert (t, h, n, act) == (typ, head, int(rec[3]), int(s["free_log_action"][i])), (i, log[1])
            assert abs(float(p) - float(rec[2])) <= 1e-5
        with torch.no_grad():
            out2 = pol.act(obs, None, None, masks, deterministic=True, return_entropy=True)
        assert len(out2) == 5 and abs(float(out2[4]) - float(entropy)) <= 1e-6
    # forced type: no type tuple
    j = int(np.flatnonzero(s["forced_log_head"] >= 0)[0])
    i, t = int(s["forced_rows"][j]), int(s["forced_type"][j])
    obs = reference_api.obs_flat_to_dict(x["obs_f"][i:i + 1], x["lists"][i:i + 1])
    with torch.no_grad():
        out = pol.act(obs, None, None, reference_api.masks_flat_to_list(x["masks"][i:i + 1]), deterministic=True,
                      condition_on_action_type=t, log_specific_action_output=True)
    log = out[5]
    assert len(log) == 1 and log[0][0] == t and log[0][1] == int(s["forced_log_head"][j])
    assert abs(float(out[4]) - float(s["forced_entropy"][j])) <= 1e-5


def test_reference_api_batch_entropy_is_mean_of_rows():
    net, x, s = _load()
    pol = reference_api.SettlersAgentPolicy(net, autocast_dtype=None)
    obs = reference_api.obs_flat_to_dict(x["obs_f"], x["lists"])
    with torch.no_grad():
        out = pol.act(obs, None, None, reference_api.masks_flat_to_list(x["masks"]), deterministic=True, return_entropy=True)
    with torch.no_grad():
        ent = net.act(x["obs_f"], x["lists"], x["lens"], x["masks"], deterministic=True, return_entropy=True)[3]
    assert np.abs(ent.numpy() - s["free_entropy"]).max() <= 1e-5
    assert abs(float(out[4]) - float(ent.double().mean())) <= 1e-6


def test_abi_refuses_bad_statistics_arguments():
    from settlers_of_catan_rl_amd import _lib
    L = _lib.lib()
    rc = L.catan_head_chain_ex(None, 1536, None, None, 1e-5, 0, 0, None, None, None, None, None, None, None, None, None, 2, 64, None)
    assert rc != 0 and "unknown flags" in L.catan_last_error().decode()
    rc = L.catan_head_chain_ex(None, 1536, None, None, 1e-5, 0, 0, None, None, None, None, None, None, None, None, None, 1, 64, None)
    assert rc != 0 and "catan_head_chain_ex: bad arguments" in L.catan_last_error().decode()
    rc = L.catan_head_fwd_entropy(None, 128, None, 0, 0, None, None, 1e-5, 13, None, 13, None, None, None, None, 64, None)
    assert rc != 0 and "entropy is NULL" in L.catan_last_error().decode()
