"""Shared by the CPU and GPU whole-update tests: tests/golden/ppo_update.npz (tools/gen_golden.py gen_ppo_update) holds what the
reference's own PPO.update did to the fixture net - two updates of 2 epochs x 4 minibatches on rollouts r0 and r1 of
rollout_small.npz - and this module runs this package's learners (`reference_api.PPO`, `train.PPOTrainer`) on the same data with
the same permutations, records the same quantities per optimiser step and compares them.

Recorded per optimiser step k (16 of them): the losses (value loss x value_loss_coef, action loss, entropy x entropy_coef), the
pre-clip gradient norm, per parameter whether its gradient is None, whether the step moved it, the gradient's norm and hashed
projection, and the norm and hashed projection of theta_k - theta_0 (policy_fixture.projection).  The fixture stores all of it twice:
the reference in fp32 and in fp64; the spread between those two is the yardstick of the tolerances."""
import numpy as np
import torch

import golden_util as gu
import policy_fixture as pf
import rollout_fixture as rf

SALT = "ppo:"


def load():
    return gu.load("ppo_update.npz")


def param_names(g):
    return [str(n) for n in g["param_names"]]


def bits(g, key, n):
    return np.unpackbits(g[key], axis=1, bitorder="little")[:, :n].astype(bool)


def fixture_policy(g, device):
    """CatanPolicy with the fixture's weights (crc32 of every tensor checked against what the generator loaded into the reference)"""
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    net = CatanPolicy()
    names = param_names(g)
    own = net.state_dict()
    assert sorted(own) == names, "parameter names differ from the reference net's"
    sd = pf.fixture_state_dict({k: tuple(own[k].shape) for k in names}, SALT)
    for k, want in zip(names, g["param_crc"]):
        assert pf.tensor_crc(sd[k]) == int(want), f"fixture weight {k} differs from the generator's"
    net.load_state_dict(sd, strict=True)
    return net.to(device)


def replay_storages(make_env, g):
    """rollout_small replayed through reference_api.SubProcGameManager on the env make_env(n, seed) (every rollout checked against
    the reference's tensors by rollout_fixture.check_rollout_fixture); -> copies of the storages of the rollouts the fixture
    updates on, with its actions (the trade heads' unused columns made legal, see the generator) and its old log-probs"""
    from settlers_of_catan_rl_amd.rollout import RolloutStorage
    want = [int(r) for r in g["rollouts"]]
    kept = {}

    def keep(r, bp, _ro):
        if r in want:
            st = bp.storage
            c = RolloutStorage(st.T, st.N, st.obs_f.device, obs_dtype=st.obs_f.dtype)
            for k in ("obs_f", "lists", "lens", "masks", "rewards", "actions", "action_log_probs", "action_masks"):
                getattr(c, k).copy_(getattr(st, k))
            kept[r] = c
    rf.check_rollout_fixture(make_env, on_rollout=keep)
    out = []
    for u, r in enumerate(want):
        st = kept[r]
        acts = torch.from_numpy(g[f"u{u}_actions"].astype(np.int64)).to(st.actions.device)
        differ = (acts != st.actions).any(-1)
        assert int(differ.sum()) > 0 and bool((acts[:, :, 0] == st.actions[:, :, 0]).all())     # (only unused trade-head columns differ)
        st.actions.copy_(acts)
        st.action_log_probs.copy_(torch.from_numpy(g[f"u{u}_old_log_probs"]).to(st.action_log_probs.device))
        out.append(st)
    return out


class _Args(object):
    def __init__(self, g):
        for k in ("clip_param", "ppo_epoch", "num_mini_batch", "value_loss_coef", "entropy_coef_start", "max_grad_norm", "recompute_returns",
                  "gamma", "gae_lambda", "lr", "eps", "truncated_seq_len"):
            setattr(self, k, g["arg_" + k].item())


def run(g, learner, net, storages, monkeypatch, autocast_dtype=None, compact=False, skip_none_grads=False, entropy_scale=1.0,
        drop_row_step=None):
    """Two updates of `learner` ("ppo": reference_api.PPO over its BatchProcessor, "trainer": train.PPOTrainer) on `storages` with the
    fixture's permutations and learning rates.  The loss back-ends in use are whatever the caller installed (torch forms on the CPU,
    the kernels on the device).  The perturbations are for the sensitivity checks: skip_none_grads (parameters without a gradient take
    no step: the behaviour before FusedAdam's none_grad_is_zero), entropy_scale (x entropy_coef), drop_row_step (that step's loss
    leaves out the minibatch's first row).  -> record dict (see the module docstring)"""
    from settlers_of_catan_rl_amd import ppo as ppo_mod
    from settlers_of_catan_rl_amd import reference_api as ra
    from settlers_of_catan_rl_amd import train
    names = param_names(g)
    args = _Args(g)
    dev = next(net.parameters()).device
    heads = net.action_head_module
    if compact:
        monkeypatch.setattr(heads, "compact_min_rows", 0, raising=False)
    else:
        monkeypatch.setattr(heads, "compact_evaluate", False, raising=False)
    prm = dict(net.named_parameters())
    theta0 = {k: prm[k].detach().clone() for k in names}
    rec = {k: [] for k in ("al", "vl", "ent", "norm", "g_none", "g_norm", "g_proj", "moved", "d_norm", "d_proj")}
    step_no = [0]

    # the fixture's permutations, one per epoch
    perms = iter(g["perms"])
    randperm0 = torch.randperm

    def randperm(n, *a, **kw):
        p = next(perms)
        assert n == len(p)
        return torch.from_numpy(p.copy()).to(kw.get("device") or "cpu")
    monkeypatch.setattr(torch, "randperm", randperm)

    # losses: the parts the loss back-end returns, the entropy evaluate_actions returns
    def wrap_loss(f):
        def loss(lp, v, old_lp, adv, v_old, ret, *a, **kw):
            if drop_row_step is not None and step_no[0] == drop_row_step:
                lp, v, old_lp, adv, v_old, ret = (x.reshape(-1)[1:] for x in (lp, v, old_lp, adv, v_old, ret))
            out, parts = f(lp, v, old_lp, adv, v_old, ret, *a, **kw)
            rec["al"].append(float(parts[0])); rec["vl"].append(float(parts[1]))
            return out, parts
        return loss
    if learner == "ppo":
        monkeypatch.setattr(ra, "_LOSS", wrap_loss(ra._LOSS))
    else:
        monkeypatch.setattr(ppo_mod, "ppo_loss", wrap_loss(ppo_mod.ppo_loss))
    ev0 = net.evaluate_actions

    def evaluate_actions(*a, **kw):
        res = ev0(*a, **kw)
        rec["ent"].append(float(res[2].detach()))
        return res
    monkeypatch.setattr(net, "evaluate_actions", evaluate_actions, raising=False)

    if learner == "ppo":
        ac = ra.SettlersAgentPolicy(net, autocast_dtype=autocast_dtype).to(dev)
        agent = ra.PPO(ac, args)
        agent.entropy_coef = args.entropy_coef_start * entropy_scale
        entropy_coef = agent.entropy_coef
        opt = agent.optimiser
    else:
        cfg = train.PPOConfig(lr=args.lr, eps=args.eps, gamma=args.gamma, gae_lambda=args.gae_lambda, clip_param=args.clip_param,
                              ppo_epoch=args.ppo_epoch, num_mini_batch=args.num_mini_batch, value_loss_coef=args.value_loss_coef,
                              entropy_coef=args.entropy_coef_start * entropy_scale, max_grad_norm=args.max_grad_norm)
        trainer = train.PPOTrainer(net, cfg, autocast_dtype=autocast_dtype)
        entropy_coef = cfg.entropy_coef
        opt = trainer.optimiser
    if skip_none_grads:
        opt.none_grad_is_zero = False
    step0 = opt.step

    def step(*a, **kw):
        rec["g_none"].append([prm[k].grad is None for k in names])
        rec["g_norm"].append([float(prm[k].grad.double().norm()) if prm[k].grad is not None else 0.0 for k in names])
        rec["g_proj"].append([pf.projection(k, prm[k].grad) if prm[k].grad is not None else 0.0 for k in names])
        before = {k: prm[k].detach().clone() for k in names}
        r = step0(*a, **kw)
        rec["norm"].append(float(opt.last_norm.reshape(-1)[0]))
        with torch.no_grad():
            rec["moved"].append([not torch.equal(before[k], prm[k]) for k in names])
            d = {k: prm[k].detach() - theta0[k] for k in names}
            rec["d_norm"].append([float(d[k].double().norm()) for k in names])
            rec["d_proj"].append([pf.projection(k, d[k]) for k in names])
        step_no[0] += 1
        return r
    monkeypatch.setattr(opt, "step", step, raising=False)

    returned = []
    for u, st in enumerate(storages):
        opt.param_groups[0]["lr"] = float(g["lrs"][u])
        if learner == "ppo":
            bp = ra.BatchProcessor(types_ns(T=st.T, N=st.N, gamma=args.gamma, gae_lambda=args.gae_lambda), lstm_dim=256, device=dev)
            bp.storage, bp._list_pad = st, [max(1, int(v)) for v in st.lens[:st.T + 1].reshape(-1, 5).max(0).values.tolist()]
            returned.append(agent.update(bp))
        else:
            returned.append(trainer.update(st))
    monkeypatch.setattr(torch, "randperm", randperm0)
    S = len(rec["norm"])
    assert len(rec["al"]) == S and len(rec["ent"]) == S
    out = {"step_losses": np.stack([np.array(rec["vl"]) * args.value_loss_coef, np.array(rec["al"]), np.array(rec["ent"]) * entropy_coef], 1),
           "update_losses": np.array(returned, dtype=np.float64), "grad_norm_total": np.array(rec["norm"])}
    for k in ("g_none", "moved"):
        out[k] = np.array(rec[k], dtype=bool)
    for k in ("g_norm", "g_proj", "d_norm", "d_proj"):
        out[k] = np.array(rec[k], dtype=np.float64)
    return out


def types_ns(T, N, gamma, gae_lambda):
    import types
    return types.SimpleNamespace(num_steps=T, num_processes=1, num_envs_per_process=N, gamma=gamma, gae_lambda=gae_lambda)


def spread(g):
    """The reference's own fp32 noise: fp32 against fp64, per compared quantity (the largest over the steps)"""
    return deviations({"step_losses": g["f32_step_losses"], "update_losses": g["f32_update_losses"], "grad_norm_total": g["f32_grad_norm_total"],
                       "g_norm": g["f32_g_norm"], "g_proj": g["f32_g_proj"], "d_norm": g["f32_d_norm"], "d_proj": g["f32_d_proj"],
                       "moved": bits(g, "f32_moved", len(param_names(g)))}, g, "f64")


def deviations(rec, g, tag="f32"):
    """the largest deviations of a record from the fixture's `tag` run: losses relative to max(|x|, 1); the pre-clip norm relative;
    per parameter the gradient's and theta_k - theta_0's norm and projection relative to that parameter's own norm (reference),
    floored at 1e-2 (gradients) / 1e-3 (theta_k - theta_0) of the step's largest (a parameter with a tiny gradient is not held to its
    own scale); the gradients of steps from GRAD_TIGHT_STEPS on separately (`*_late`); the parameters whose moved flag differs"""
    S = len(g[f"{tag}_grad_norm_total"])
    assert len(rec["grad_norm_total"]) == S, (len(rec["grad_norm_total"]), S)
    rel = lambda a, b: np.abs(a - b) / np.maximum(np.abs(b), 1.0)
    out = {"step_losses": float(rel(rec["step_losses"], g[f"{tag}_step_losses"]).max()),
           "update_losses": float(rel(rec["update_losses"], g[f"{tag}_update_losses"]).max()),
           "grad_norm_total": float((np.abs(rec["grad_norm_total"] - g[f"{tag}_grad_norm_total"]) / g[f"{tag}_grad_norm_total"]).max())}
    for which, floor in (("g", 1e-2), ("d", 1e-3)):
        ref_n = g[f"{tag}_{which}_norm"]
        den = np.maximum(ref_n, floor * ref_n.max(1, keepdims=True))
        dn = np.abs(rec[f"{which}_norm"] - ref_n) / den
        dp = np.abs(rec[f"{which}_proj"] - g[f"{tag}_{which}_proj"]) / den
        if which == "g":                  # the gradients: tight before the kink flip (see GRAD_TIGHT_STEPS), loose from there on
            k = GRAD_TIGHT_STEPS
            out["g_norm_late"], out["g_proj_late"] = float(dn[k:].max()), float(dp[k:].max())
            dn, dp = dn[:k], dp[:k]
        out[f"{which}_norm"] = float(dn.max())
        out[f"{which}_proj"] = float(dp.max())
        out[f"{which}_worst"] = (int(dp.max(1).argmax()), param_names(g)[int(dp.max(0).argmax())])
    want_moved = bits(g, f"{tag}_moved", len(param_names(g)))
    out["moved_mismatch"] = int(((np.asarray(rec["moved"]) != want_moved) & ~rounding_only(g)[None, :]).sum())
    return out


def rounding_only(g):
    """parameters whose gradient is zero in exact arithmetic (the attention's key biases: softmax does not see a shift of all the
    scores): in fp64 non-zero but below 1e-12 of the largest in every step.  In fp32 they carry rounding noise of ~1e-9, and whether an Adam
    step of that noise changes the fp32 value at all is itself noise: they are left out of the comparison of the moved sets"""
    r = (g["f64_g_norm"] / g["f64_g_norm"].max(1, keepdims=True)).max(0)
    return (r > 0) & (r < 1e-12)


# The gradients are held tight (8 x the reference's own spread, floor 1e-4) in steps 0 .. 13.  In step 14 one ReLU unit of
# value_network_fc_1 sits within rounding noise of its kink on some row: theta_14 of this package and of the reference differ at the
# noise level only, yet the unit is on in one and off in the other, and that row's value-net gradient changes by a finite amount
# (measured: <= 3.6e-5 in steps 0 .. 13 against the fp32 reference, 4.5e-3 in step 14, 6.9e-4 in step 15; no clip or max branch of
# the loss is near its tie there).  From step 14 on the gradients are held to 1e-2; theta_k - theta_0 stays tight in every step
GRAD_TIGHT_STEPS = 14

# the tolerances, as multiples of the reference's own fp32-against-fp64 spread (`spread`), with floors
TOL_FACTOR = 8.0
TOL_FLOOR = {"step_losses": 2e-5, "update_losses": 2e-5, "grad_norm_total": 1e-4, "g_norm": 1e-4, "g_proj": 1e-4, "g_norm_late": 1e-2,
             "g_proj_late": 1e-2, "d_norm": 5e-4, "d_proj": 5e-4}


def tolerances(g, factor=1.0):
    s = spread(g)
    return {k: factor * max(TOL_FACTOR * s[k], fl) for k, fl in TOL_FLOOR.items()}


def check(rec, g, factor=1.0):
    """-> (ok, deviations, tolerances)"""
    dev = deviations(rec, g)
    tol = tolerances(g, factor)
    ok = dev["moved_mismatch"] == 0 and all(dev[k] <= tol[k] for k in tol)
    return ok, dev, tol

