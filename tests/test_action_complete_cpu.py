"""The action-row completion rule on the CPU: why it is needed and what it guarantees.

An action row that did not come out of the net - the rule-based player's, the uniform-random sampler's - fills only the columns its
type uses; `_ActionHeads.forward` evaluates every head on every row and multiplies the unused ones by 0, and 0 is often illegal
under such a head's mask: -inf x 0 = NaN.  The completion (tests/action_complete_reference.py, the twin of
catan_complete_action_rows) puts a legal index into every unused column."""
import numpy as np
import pytest
import torch

import action_complete_reference as acr
import scripted_reference as sr
from oracle_vec_env import OracleVecEnv, ScriptedPolicy as RandomPolicy
from settlers_of_catan_rl_amd.policy import CatanPolicy

N, SEED, STEPS, EVERY = 64, 5, 200, 8


def play(n=N, seed=SEED, steps=STEPS, every=EVERY):
    """The play the GPU test repeats: lock-step, even games stepped with the rule-based player's action, odd games with the oracle's
    uniform-random one; every `every`-th step both kinds of row are kept for all games.  -> dict of arrays, rows = 2 n per kept step
    (the scripted rows, then the random ones) with their observations and masks."""
    env = OracleVecEnv(n, seed=seed)
    rnd = RandomPolicy(env)
    keep = {k: [] for k in ("f", "lists", "lens", "masks", "rows", "kind")}
    types = np.zeros((2, 13), dtype=np.int64)                # the types decided over the whole play: scripted, random
    for it in range(steps):
        f, lists, lens = env.get_obs()
        masks = env.get_action_masks()
        scripted, _ = sr.decide_all(env.export_state().numpy(), masks.numpy())
        _, ra, _ = rnd.act(f, lists, lens, masks)
        np.add.at(types[0], np.asarray(scripted)[:, 0], 1)
        np.add.at(types[1], ra.numpy()[:, 0], 1)
        if it % every == 0:
            for kind, rows in ((0, scripted), (1, ra.numpy())):
                keep["f"].append(f.numpy()); keep["lists"].append(lists.numpy()); keep["lens"].append(lens.numpy())
                keep["masks"].append(masks.numpy()); keep["rows"].append(np.asarray(rows, dtype=np.int64))
                keep["kind"].append(np.full(n, kind))
        a = ra.clone()
        a[::2] = torch.from_numpy(np.asarray(scripted[::2], dtype=np.int64))
        env.step(a.to(torch.int32))
    out = {k: np.concatenate(v) for k, v in keep.items()}
    out["types"] = types
    return out


@pytest.fixture(scope="module")
def rows(oracle):
    d = play()
    d["res"] = d["f"][:, 12:18]
    d["lo"] = acr.complete_all(d["rows"], d["masks"], d["res"])
    d["hi"] = acr.complete_all(d["rows"], d["masks"], d["res"], highest=True)
    torch.manual_seed(0)
    net = CatanPolicy().eval()
    F, L, NL, M = (torch.from_numpy(d[k]) for k in ("f", "lists", "lens", "masks"))

    def logp(a):
        with torch.no_grad():
            return net.evaluate_actions(F, L, NL.long(), M, torch.from_numpy(a))[1][:, 0]
    d["logp"] = logp
    return d


def test_the_play_shows_every_type(rows):
    """over its 200 steps: all 13 types among the random rows, 12 among the scripted ones (the player never proposes a trade)"""
    scr_types, rnd_types = (set(np.flatnonzero(t).tolist()) for t in rows["types"])
    assert rnd_types == set(range(13)), sorted(rnd_types)
    assert scr_types == set(range(13)) - {acr.PROPOSE}, sorted(scr_types)


def test_raw_rows_are_not_teacher_forceable(rows):
    """the need: rows as the samplers leave them give non-finite joint log-probs"""
    lp = rows["logp"](rows["rows"])
    bad = ~torch.isfinite(lp)
    print("non-finite raw rows: scripted %d of %d, random %d of %d" % (int(bad[rows["kind"] == 0].sum()), int((rows["kind"] == 0).sum()),
                                                                       int(bad[rows["kind"] == 1].sum()), int((rows["kind"] == 1).sum())))
    assert int(bad.sum()) >= 1


def test_completed_rows_are_finite_and_keep_their_used_columns(rows):
    lo, raw = rows["lo"], rows["rows"]
    lp = rows["logp"](lo)
    assert bool(torch.isfinite(lp).all()), int((~torch.isfinite(lp)).sum())
    for i in range(len(raw)):
        used = sorted(acr.used_columns(raw[i]))
        assert np.array_equal(lo[i][used], raw[i][used]) and np.array_equal(rows["hi"][i][used], raw[i][used]), (i, raw[i], lo[i])


def test_log_prob_does_not_depend_on_the_legal_filler(rows):
    """bit-equal whether the unused columns hold the lowest or the highest legal index"""
    assert int((rows["lo"] != rows["hi"]).any(1).sum()) > len(rows["lo"]) // 2        # (the two completions do differ)
    lp_lo, lp_hi = rows["logp"](rows["lo"]), rows["logp"](rows["hi"])
    assert torch.equal(lp_lo, lp_hi)


def test_rows_outside_the_types_are_left_alone():
    row = np.arange(18) - 1
    assert np.array_equal(acr.complete(row, np.ones(325, dtype=np.float32), np.ones(6)), row)
    row[0] = 13
    assert np.array_equal(acr.complete(row, np.ones(325, dtype=np.float32), np.ones(6)), row)
