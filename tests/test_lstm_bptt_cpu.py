"""Truncated-BPTT minibatches (train.lstm_minibatches) against the reference's `BatchProcessor.generator_lstm`
(RL/ppo/process_batch.py:203-293) on a tagged storage, and the LSTM value re-evaluation rule of
`compute_advantages_alt` (process_batch.py:112-128), both as recorded from the reference (tests/golden/ref_checks.npz); the index
arithmetic is also checked reference-free."""
import numpy as np
import pytest
import torch

import golden_util
from settlers_of_catan_rl_amd.train import lstm_minibatches


def test_pieces_cover_every_decision_once():
    T, N, L, nmb = 20, 12, 5, 8
    perm = torch.randperm(N * T // L, generator=torch.Generator().manual_seed(0))
    seen = torch.zeros(T, N, dtype=torch.int64)
    nb = 0
    for t, g in lstm_minibatches(T, N, L, nmb, perm):
        assert t.shape == (L, (T * N) // nmb // L) and g.shape == (t.shape[1],)
        assert torch.equal(t[1:] - t[:-1], torch.ones_like(t[1:])) and bool((t[0] % L == 0).all())
        seen[t, g[None, :].expand_as(t)] += 1
        nb += 1
    assert nb == nmb and bool((seen == 1).all())
    with pytest.raises(ValueError):
        list(lstm_minibatches(21, N, L, nmb, perm))
    with pytest.raises(ValueError):
        list(lstm_minibatches(T, N, L, 5, perm))      # 9 pieces per minibatch do not divide 48


def test_minibatches_equal_reference_generator():
    """The reference generator's minibatches over a tagged storage (value = 100 t + game; tests/golden/ref_checks.npz,
    tools/gen_golden.py gen_ref_checks), field by field, against the storage gathered at lstm_minibatches' indices."""
    fx = golden_util.load("ref_checks.npz")
    T, N, L, nmb = 20, 6, 5, 4
    tag = (torch.arange(T + 1)[:, None] * 100 + torch.arange(N)[None, :]).float()          # value = 100 t + game
    obs_a, obs_b = tag[:, :, None] + torch.tensor([0.0, 0.25]), tag[:, :, None] * 2
    hidden = (tag[:, :, None] + torch.tensor([0.1, 0.2, 0.3]), -tag[:, :, None] - torch.tensor([0.1, 0.2, 0.3]))
    actions = [tag[:T, :, None].long() + i for i in range(3)]
    action_masks = [tag[:T, :, None] + 0.5, torch.stack([tag[:T, :, None] + 1, tag[:T, :, None] + 2])]
    values, returns = tag[:, :, None] + 7, tag[:T, :, None] + 8
    masks = torch.from_numpy(fx["bptt_masks"])
    action_log_probs, advantages = tag[:T, :, None] + 9, tag[:T, :, None] + 10
    np.random.seed(5)
    perm = torch.from_numpy(np.random.permutation(N * T // L))                               # the generator's only draw (:216)
    mine = list(lstm_minibatches(T, N, L, nmb, perm))
    ref = {k[len("bptt_"):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("bptt_") and k != "bptt_masks"}
    assert len(mine) == len(ref["obs_a"]) == nmb
    for i, (t, gm) in enumerate(mine):
        rows_t, rows_g = t.reshape(-1), gm[None, :].expand_as(t).reshape(-1)
        assert torch.equal(ref["obs_a"][i], obs_a[rows_t, rows_g]) and torch.equal(ref["obs_b"][i], obs_b[rows_t, rows_g])
        assert torch.equal(ref["hid0"][i], hidden[0][t[0], gm]) and torch.equal(ref["hid1"][i], hidden[1][t[0], gm])
        for j in range(3):
            assert torch.equal(ref[f"act{j}"][i], actions[j][rows_t, rows_g])
        assert torch.equal(ref["amask0"][i], action_masks[0][rows_t, rows_g]) and torch.equal(ref["amask1"][i], action_masks[1][:, rows_t, rows_g])
        assert torch.equal(ref["vpred"][i], values[rows_t, rows_g]) and torch.equal(ref["ret"][i], returns[rows_t, rows_g])
        assert torch.equal(ref["msk"][i], masks[rows_t, rows_g]) and torch.equal(ref["oldlp"][i], action_log_probs[rows_t, rows_g])
        assert torch.equal(ref["adv"][i], advantages[rows_t, rows_g])


def test_lstm_value_reevaluation_rule():
    """compute_advantages_alt with an LSTM net (tests/golden/ref_checks.npz, tools/gen_golden.py gen_ref_checks): every stored
    decision is ONE step from its stored state with its own terminal mask (the hidden rows equal the input rows,
    policy.py:117-123) - what PPOTrainer.compute_values restates."""
    fx = golden_util.load("ref_checks.npz")
    T, N = 4, 3
    obs, h, c, masks = (torch.from_numpy(fx[k]) for k in ("vre_obs", "vre_h", "vre_c", "vre_masks"))
    assert int(fx["vre_call_rows"].sum()) == (T + 1) * N
    # the rows the reference evaluated: each stored (observation, state, terminal mask), once
    called = torch.cat([torch.from_numpy(fx[k]) for k in ("vre_call_obs", "vre_call_h", "vre_call_c", "vre_call_masks")], 1)
    stored = torch.cat([obs, h, c, masks], -1).reshape((T + 1) * N, -1)
    assert sorted(map(tuple, called.tolist())) == sorted(map(tuple, stored.tolist()))
    want = obs.sum(-1, keepdim=True) + (h * masks).sum(-1, keepdim=True)
    assert torch.allclose(torch.from_numpy(fx["vre_values"]), want)
