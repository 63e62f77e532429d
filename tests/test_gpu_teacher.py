"""GPU: kickstarting from the rule-based player (csrc/catan_players.hip) - catan_complete_action_rows against its numpy
twin (tests/action_complete_reference.py), teacher labels in the rollout collector's loops, catan_imitation_loss against fp64,
evaluate_actions(teacher_actions=) against the CPU, and one PPO update with the imitation term."""
import copy
import math

import numpy as np
import pytest
import torch

import action_complete_reference as acr
import policy_fixture as pf
import rollout_fixture as rf
import scripted_reference as sr
from guarded import ptr as P, stream as _stream

pytestmark = pytest.mark.gpu

N, SEED = 64, 5
STORAGE_KEYS = ("obs_f", "lists", "lens", "masks", "rewards", "actions", "action_log_probs", "action_masks")


def _env(n, seed, **kw):
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    return VecCatanEnv(n, seed=seed, **kw)


# ---------------------------------------------------------------------------------------------- 1. the completion kernel
def test_kernel_equals_the_twin_over_200_steps(hip_lib):
    """The play of tests/test_action_complete_cpu.py on the device, every step: the rule-based player's rows and the uniform-random
    sampler's, completed by the kernel, equal the twin's completion of the same rows from get_action_masks() and obs_f[12:18] - all 18
    words.  Even games step the player's action, odd games the random one."""
    env = _env(N, SEED)
    even = (torch.arange(N, device="cuda") % 2 == 0)[:, None]
    types, changed = np.zeros((2, 13), dtype=np.int64), 0
    for step in range(200):
        masks = env.get_action_masks().cpu().numpy()
        res = env.get_obs()[0][:, 12:18].float().cpu().numpy()
        scripted, rnd = env.sample_scripted_actions(), env.sample_random_actions(step)
        want_s, _ = sr.decide_all(env.export_state().cpu().numpy(), masks)
        assert np.array_equal(scripted.cpu().numpy(), want_s)
        for kind, raw in ((0, scripted), (1, rnd)):
            raw_h = raw.cpu().numpy()
            got = env.complete_action_rows(raw.clone()).cpu().numpy()
            want = acr.complete_all(raw_h, masks, res)
            bad = np.flatnonzero((got != want).any(1))
            assert bad.size == 0, (step, kind, int(bad[0]), raw_h[bad[0]].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())
            np.add.at(types[kind], raw_h[:, 0], 1)
            changed += int((got != raw_h).any(1).sum())
        env.step(torch.where(even, scripted, rnd))
    assert env.invalid_action_count() == 0
    print("types completed: scripted", types[0].tolist(), "random", types[1].tolist(), "rows changed", changed)
    assert (types[1] > 0).all() and (np.delete(types[0], acr.PROPOSE) > 0).all() and types[0][acr.PROPOSE] == 0
    assert changed > 200 * N


def test_label_is_the_completed_scripted_action_and_lists_are_honoured(hip_lib):
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy
    env = _env(N, SEED)
    env.random_rollout(0, 150)
    full = env.complete_action_rows(env.sample_scripted_actions())
    bot = ScriptedPolicy(env)
    assert torch.equal(bot.label(), full) and bot.label().dtype == torch.int32
    # a list with duplicates, negative and out-of-range ids: those rows stay exactly as given
    games = torch.tensor([3, 3, -1, 63, N, 0, -7, 3], dtype=torch.int32, device="cuda")
    raw = env.sample_scripted_actions(games=games)                       # (EndTurn placeholders for the ids outside the handle)
    raw[2] = 77; raw[4] = -5
    got = env.complete_action_rows(raw.clone(), games=games)
    assert torch.equal(got[[0, 1, 3, 5, 7]], full[[3, 3, 63, 0, 3]]) and torch.equal(got[[2, 4, 6]], raw[[2, 4, 6]])
    assert torch.equal(bot.label(games=games.long())[[0, 1, 3, 5, 7]], full[[3, 3, 63, 0, 3]])      # (an int64 list is converted)
    # a row of type -1 (the env's no-op) or 13 is not a row of the table
    rows = full.clone()
    rows[5] = torch.arange(18, dtype=torch.int32, device="cuda") - 1
    rows[9, 0] = 13
    before = rows.clone()
    got = env.complete_action_rows(rows)
    assert got is rows and torch.equal(got[[5, 9]], before[[5, 9]]) and torch.equal(got, before)    # (completion is idempotent on the rest)


def test_waiting_games_are_left_alone(hip_lib):
    """inside a catan_step_deferred sequence (window 4) the rows of the games that wait for their step keep every word; the others are
    completed (an EndTurn row uses no column: all 17 are rewritten, none can keep the sentinel 77)"""
    env = _env(N, SEED + 1)
    sentinel = torch.full((N, 18), 77, dtype=torch.int32, device="cuda")
    sentinel[:, 0] = acr.ENDTURN
    seen_waiting = seen_done = 0
    for _ in range(300):
        _, _, status = env.step_deferred(env.sample_scripted_actions(), window=4)
        waiting = status.bool()
        got = env.complete_action_rows(sentinel.clone())
        assert torch.equal(got[waiting], sentinel[waiting])
        assert bool((got[~waiting][:, 1:] != 77).all())
        seen_waiting += int(waiting.sum()); seen_done += int((~waiting).sum())
    env.step_flush()
    print("rows of waiting games:", seen_waiting, "of stepping games:", seen_done)
    assert seen_waiting > 0 and env.invalid_action_count() == 0


def test_bad_arguments_name_the_entry_point(hip_lib):
    L = hip_lib
    env = _env(N, 0)
    out = torch.zeros((128, 18), dtype=torch.int32, device="cuda")

    def err(rc):
        assert rc == -1                                  # CATAN_EINVAL (include/catan_hip.h)
        return L.catan_last_error().decode()
    assert "catan_complete_action_rows" in err(L.catan_complete_action_rows(None, None, 64, P(out), _stream()))
    assert "catan_complete_action_rows" in err(L.catan_complete_action_rows(env.h, None, 64, None, _stream()))
    assert "catan_complete_action_rows" in err(L.catan_complete_action_rows(env.h, None, 0, P(out), _stream()))
    assert "catan_complete_action_rows" in err(L.catan_complete_action_rows(env.h, None, 65, P(out), _stream()))
    assert L.catan_complete_action_rows(env.h, None, 64, P(out), _stream()) == 0
    # catan_collector_label: every pointer is needed (waiting_before alone may be NULL)
    cnt = torch.zeros((4, N), dtype=torch.int64, device="cuda"); fl = torch.zeros((4, N), dtype=torch.uint8, device="cuda")
    pid = torch.ones(N, dtype=torch.int64, device="cuda"); dec = torch.ones(N, dtype=torch.int32, device="cuda")
    st = torch.zeros((8, N, 18), dtype=torch.int16, device="cuda")
    good = [P(cnt), P(fl), P(pid), P(dec), P(out), P(st)]
    for k in range(6):
        assert "catan_collector_label" in err(L.catan_collector_label(N, 8, *(good[:k] + [None] + good[k + 1:]), None, _stream()))
    assert "catan_collector_label" in err(L.catan_collector_label(0, 8, *good, None, _stream()))
    assert "catan_collector_label" in err(L.catan_collector_label(N, 0, *good, None, _stream()))
    assert L.catan_collector_label(N, 8, *good, None, _stream()) == 0            # (live is all zero: nothing is stored)
    # catan_imitation_loss
    lp = torch.zeros(8, device="cuda"); rows = torch.zeros((8, 18), dtype=torch.int64, device="cuda")
    loss = torch.zeros(1, device="cuda"); dlp = torch.zeros(8, device="cuda")
    block = torch.zeros(33, dtype=torch.float64, device="cuda")
    ws = torch.zeros(L.catan_imitation_loss_workspace_doubles(), dtype=torch.float64, device="cuda")
    good = [P(lp), P(rows), 8, P(loss), P(dlp), P(block), P(ws)]
    for k in (0, 1, 3, 4, 5, 6):
        assert "catan_imitation_loss" in err(L.catan_imitation_loss(*(good[:k] + [None] + good[k + 1:]), _stream()))
    assert "catan_imitation_loss" in err(L.catan_imitation_loss(*(good[:2] + [0] + good[3:]), _stream()))
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(st)) == 0 and int(torch.count_nonzero(block)) == 0 and int(torch.count_nonzero(ws)) == 0


# ---------------------------------------------------------------------------------------------- 2. the collector
class SpyEnv(object):
    """delegates to the env and keeps, for every catan_step, the games as they were decided in"""

    def __init__(self, env):
        self.env, self.log = env, []

    def step(self, a):
        env = self.env
        self.log.append((env.export_state().cpu().numpy(), env.get_action_masks().cpu().numpy(), env.get_obs()[0][:, 12:18].float().cpu().numpy(),
                         env.deciding_player().cpu().numpy(), (a[:, 0] >= 0).cpu().numpy()))
        return env.step(a)

    def __getattr__(self, name):
        return getattr(self.env, name)


def _collect(T, gathers, fused, teacher, spy=False, **ckw):
    from test_gpu_collector import SamplerPolicy
    from settlers_of_catan_rl_amd.rollout import RolloutCollector
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy
    env = _env(N, SEED)
    env.random_rollout(0, 150)
    inner = SpyEnv(env) if spy else env
    cenv = rf.CountingEnv(inner)
    col = RolloutCollector(cenv, SamplerPolicy(cenv), T, seed=SEED, teacher=ScriptedPolicy(env) if teacher else None, **ckw)
    col.fused_bookkeeping = fused
    out = []
    for _ in range(gathers):
        first = len(inner.log) if spy else 0
        st = col.gather_rollouts()
        snap = {k: getattr(st, k).clone().cpu() for k in STORAGE_KEYS}
        snap["games_complete"] = st.games_complete
        snap["state"] = env.export_state().cpu()
        snap["n_act"] = col.n_act.clone().cpu()
        if teacher:
            snap["teacher_actions"] = st.teacher_actions.clone().cpu()
        if spy:
            snap["log"] = inner.log[first:]
        out.append(snap)
        col.after_rollouts()
    assert env.invalid_action_count() == 0 and env.scripted_fallback_count() == 0
    return out, col


def test_collector_labels_in_both_loops_and_schedules(hip_lib):
    """T = 8, N = 64, two rollouts: the tensor-operation loop (catan_step) and the device loop with catan_step and with window 4 store
    the same labels - the twin's for the states the stored decisions were taken in - and everything else as a collector without a
    teacher does.  Three schedules, not four: the tensor-operation loop is lock-step only (_gather_tensor steps with catan_step whatever
    deferred_window says), so "tensor loop, window 4" would be the first run again and is NOT covered - there is no such schedule."""
    T = 8
    base, col = _collect(T, 2, False, True, spy=True, deferred_window=0)
    assert col.storage.teacher_actions.dtype == torch.int16 and col.storage.teacher_actions.shape == (T, N, 18)
    plain, col0 = _collect(T, 2, False, False, deferred_window=0)
    assert col0.storage.teacher_actions is None
    active = col.active_pid.cpu().numpy()
    for snap, ref in zip(base, plain):
        for k in STORAGE_KEYS + ("games_complete", "state", "n_act"):
            assert torch.equal(snap[k], ref[k]) if torch.is_tensor(snap[k]) else snap[k] == ref[k], k
        n_act = np.zeros(N, dtype=np.int64)
        want = np.zeros((T, N, 18), dtype=np.int64)
        for blobs, masks, res, deciding, live in snap["log"]:
            for g in range(N):
                if live[g] and deciding[g] == active[g]:
                    want[min(int(n_act[g]), T - 1), g] = acr.complete(sr.decide(blobs[g], masks[g])[0], masks[g], res[g])
                    n_act[g] += 1
        assert np.array_equal(n_act, snap["n_act"].numpy())
        got = snap["teacher_actions"].numpy()
        for g in range(N):
            k = min(int(n_act[g]), T)
            assert np.array_equal(got[:k, g], want[:k, g]), (g, got[:k, g].tolist(), want[:k, g].tolist())
    for what, fused, ckw in (("device loop, catan_step", True, dict(deferred_window=0)), ("device loop, window 4", True, dict(deferred_window=4))):
        got, _ = _collect(T, 2, fused, True, **ckw)
        for g, (x, y) in enumerate(zip(base, got)):
            for k in STORAGE_KEYS + ("games_complete", "state", "n_act", "teacher_actions"):
                assert torch.equal(x[k], y[k]) if torch.is_tensor(x[k]) else x[k] == y[k], (what, "gather", g, k)


# ---------------------------------------------------------------------------------------------- 3. the loss kernel
HALF = np.float32(-0.6931472)
_CASES = {}


def _loss_case(B, seed):
    """inputs of one call and their fp64 reference (computed once, shared, never written to)"""
    if (B, seed) not in _CASES:
        rng = np.random.default_rng(seed)
        lp = (-rng.exponential(1.5, B)).astype(np.float32)
        special = [-np.inf, np.nan, 0.0, HALF, np.nextafter(HALF, np.float32(0)), np.nextafter(HALF, np.float32(-1)), np.inf, -0.0]
        k = len(special) if B >= 63 else (1 if seed >= 200 else 0)      # (B = 1: a finite row in the first call, -inf in the second)
        for v, i in zip(special[:k], rng.permutation(B)[:k]):
            lp[i] = v
        typ = rng.integers(0, 13, B)
        rows = rng.integers(0, 70, (B, 18)).astype(np.int64)
        rows[:, 0] = typ
        finite = np.isfinite(lp)
        nll = np.where(finite, -lp.astype(np.float64), 0.0)
        w = np.zeros(33)
        w[0], w[1], w[2], w[3] = B, 1, math.fsum(nll), max(0.0, float(nll.max()))
        w[4], w[5] = np.count_nonzero(finite & (lp > HALF)), np.count_nonzero(~finite)
        for t in range(13):
            w[6 + t], w[19 + t] = np.count_nonzero(finite & (typ == t)), math.fsum(nll[finite & (typ == t)])
        dlp = np.where(finite, np.float32(-1.0 / B), np.float32(0.0)).astype(np.float32)
        _CASES[(B, seed)] = dict(lp=lp, rows=rows, w=w, abs=math.fsum(np.abs(nll)), dlp=dlp, typ=typ, finite=finite, nll=nll)
    return _CASES[(B, seed)]


def _launch_loss(L, c, block, ws):
    lp, rows = torch.from_numpy(c["lp"]).cuda(), torch.from_numpy(c["rows"]).cuda()
    loss, dlp = torch.full((1,), 9.0, device="cuda"), torch.full((lp.numel(),), 9.0, device="cuda")
    assert L.catan_imitation_loss(P(lp), P(rows), lp.numel(), P(loss), P(dlp), P(block), P(ws), _stream()) == 0, L.catan_last_error()
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(ws.view(torch.int64))) == 0, "the workspace (partials and arrival counter) is all zero after every call"
    return loss.cpu().numpy(), dlp.cpu().numpy()


@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257, 4097, 70001])
def test_imitation_loss_against_fp64(hip_lib, B):
    """Two calls into one block.  Counts, the maximum and dlp exactly; the fp64 sum of a call's B rows within B * 2^-52 * sum|nll| of the
    exactly rounded sum (sequential fp64 summation is the worst order) - checked on the block after the first call; after the second the
    block holds 2 B rows, so the same bound reads 2 B * 2^-52 * (sum|nll| of both calls).  The loss within one fp32 rounding of the fp64
    mean; a repeat gives the same bits.  70 001 rows: above 256 x 256, where the grid is capped at 256 workgroups and every thread
    strides over the rows more than once - the shape of the trainer's 204 800-row minibatches."""
    L = hip_lib
    assert L.catan_imitation_loss_words() == 33
    ws = torch.zeros(L.catan_imitation_loss_workspace_doubles(), dtype=torch.float64, device="cuda")
    a, b = _loss_case(B, 100 + B), _loss_case(B, 200 + B)
    blocks = torch.zeros((3, 33), dtype=torch.float64, device="cuda")
    blocks[1] = 7.0                                                      # a neighbour's block
    for target in (0, 2):
        for c in (a, b):
            loss, dlp = _launch_loss(L, c, blocks[target], ws)
            ref = c["w"][2] / B
            assert abs(float(loss[0]) - ref) <= 2.0 ** -23 * abs(ref), (float(loss[0]), ref)
            assert np.array_equal(dlp.view(np.int32), c["dlp"].view(np.int32))
            if c is a:                                                   # one call's B rows alone: the bound as the issue states it
                first = blocks[target].cpu().numpy()
                assert abs(first[2] - a["w"][2]) <= B * 2.0 ** -52 * a["abs"], (first[2], a["w"][2])
    got = blocks[0].cpu().numpy()
    exact = [0, 1, 4, 5] + list(range(6, 19))
    assert np.array_equal(got[exact], (a["w"] + b["w"])[exact]) and got[3] == max(a["w"][3], b["w"][3]) and got[32] == 0.0
    assert abs(got[2] - math.fsum([a["w"][2], b["w"][2]])) <= 2 * B * 2.0 ** -52 * (a["abs"] + b["abs"])
    for t in range(13):
        bound = 2 * B * 2.0 ** -52 * sum(math.fsum(np.abs(c["nll"][c["finite"] & (c["typ"] == t)])) for c in (a, b))
        assert abs(got[19 + t] - (a["w"][19 + t] + b["w"][19 + t])) <= bound, t
    assert torch.equal(blocks[0].view(torch.int64), blocks[2].view(torch.int64)), "a given sequence of calls gives the same bits"
    assert torch.equal(blocks[1], torch.full((33,), 7.0, dtype=torch.float64, device="cuda"))
    if B >= 63:
        assert got[5] >= 4                                               # -inf, NaN, +inf ... were among the rows


def test_imitation_loss_through_the_package(hip_lib):
    """ppo.imitation_loss on device tensors runs the kernel (its own workspace per stream) and hands g x dlp back"""
    from settlers_of_catan_rl_amd import ppo
    c = _loss_case(257, 457)
    lp = torch.from_numpy(c["lp"]).cuda().view(-1, 1).requires_grad_(True)
    block = torch.zeros(33, dtype=torch.float64, device="cuda")
    loss = ppo.imitation_loss(lp, torch.from_numpy(c["rows"]).cuda(), block)
    (2.0 * loss).backward()
    assert lp.grad.shape == (257, 1) and np.array_equal(lp.grad.view(-1).cpu().numpy(), np.float32(2.0) * c["dlp"])
    assert abs(float(loss.detach()) - c["w"][2] / 257) <= 2.0 ** -23 * c["w"][2] / 257
    assert np.array_equal(block.cpu().numpy()[[0, 1, 4, 5]], c["w"][[0, 1, 4, 5]])
    assert int(torch.count_nonzero(ppo._imit_workspace(block.device))) == 0
    cpu_block = torch.zeros(33, dtype=torch.float64)
    cpu_loss = ppo.imitation_loss(torch.from_numpy(c["lp"]), torch.from_numpy(c["rows"]), cpu_block)          # the torch form agrees
    assert abs(float(cpu_loss) - float(loss.detach())) <= 2.0 ** -22 * abs(float(loss.detach())) and np.array_equal(cpu_block.numpy()[[0, 1, 3, 4, 5]], block.cpu().numpy()[[0, 1, 3, 4, 5]])
    with pytest.raises(ValueError):
        ppo.imitation_loss(lp, torch.from_numpy(c["rows"]).cuda(), torch.zeros(33, dtype=torch.float64))       # a host block


# ---------------------------------------------------------------------------------------------- 4. the second heads pass
@pytest.fixture(scope="module")
def labelled_rows():
    """256 decisions of a 64-game play on the device: observations, masks, the net's sampled actions and the teacher's labels"""
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy
    torch.manual_seed(3)
    net = CatanPolicy().cuda().eval()
    env = _env(N, SEED)
    bot = ScriptedPolicy(env)
    keep = {k: [] for k in ("f", "lists", "lens", "masks", "acts", "labels")}
    for step in range(160):
        if step % 40 == 39:
            f, lists, lens = env.get_obs()
            masks = env.get_action_masks()
            with torch.no_grad():
                _, a, _ = net.act(f, lists, lens.long(), masks)
            for k, v in zip(keep, (f, lists, lens.long(), masks, a, bot.label().long())):
                keep[k].append(v.clone())
        rnd = env.sample_random_actions(step)
        env.step(torch.where((torch.arange(N, device="cuda") % 2 == 0)[:, None], env.sample_scripted_actions(), rnd))
    return net, {k: torch.cat(v) for k, v in keep.items()}


@pytest.mark.parametrize("path", ["full", "compact"])
def test_evaluate_actions_with_teacher_rows_against_the_cpu(hip_lib, labelled_rows, path):
    """fp32, the bounds of tests/test_gpu_policy_fixture.py: the teacher's joint log-prob within 1e-5 (relative to max(1, |x|)) of the
    CPU's, every parameter's gradient (norm and hashed projection) within 1e-4 of its own size; the first three results are what the call
    without teacher rows returns.  compact: the per-type row sets of the learner (_evaluate_compact), forced by compact_min_rows = 1."""
    net0, x = labelled_rows
    B = x["f"].shape[0]
    cpu = copy.deepcopy(net0).cpu()
    gpu = copy.deepcopy(net0)
    if path == "compact":
        gpu.action_head_module.compact_min_rows = 1
    res = {}
    for name, net, dev in (("cpu", cpu, "cpu"), ("gpu", gpu, "cuda")):
        t = {k: v.to(dev) for k, v in x.items()}
        net.zero_grad()
        out = net.evaluate_actions(t["f"], t["lists"], t["lens"], t["masks"], t["acts"], teacher_actions=t["labels"])
        assert len(out) == 4 and out[3].shape == (B, 1) and bool(torch.isfinite(out[3]).all())
        with torch.no_grad():
            plain = net.evaluate_actions(t["f"], t["lists"], t["lens"], t["masks"], t["acts"])
        assert len(plain) == 3
        w = torch.linspace(1.5, 0.5, B, device=dev)[:, None]
        (out[3].float() * w).sum().backward()
        prm = dict(net.named_parameters())
        res[name] = (out, plain, {k: (float(p.grad.double().norm()), pf.projection(k, p.grad)) if p.grad is not None else (0.0, 0.0) for k, p in prm.items()})
    rel = lambda a, b: float(((a.float().cpu() - b.float().cpu()).abs() / b.float().cpu().abs().clamp(min=1.0)).max())
    (og, pg, gg), (oc, pc, gc) = res["gpu"], res["cpu"]
    dev = {"teacher_logp": rel(og[3], oc[3]), "logp": rel(og[1], oc[1]), "value": rel(og[0], oc[0]), "entropy": abs(float(og[2]) - float(oc[2])),
           "plain_logp": rel(pg[1], og[1]), "plain_value": rel(pg[0], og[0])}
    scale = max(v[0] for v in gc.values())
    den = {k: max(gc[k][0], 1e-3 * scale) for k in gc}
    dev["grad_norm"] = max(abs(gg[k][0] - gc[k][0]) / den[k] for k in gc)
    dev["grad_proj"] = max(abs(gg[k][1] - gc[k][1]) / den[k] for k in gc)
    print(path, "deviations from the CPU:", dev)
    assert scale > 0
    for k in ("teacher_logp", "logp", "value", "entropy", "plain_logp", "plain_value"):
        assert dev[k] <= 1e-5, (k, dev)
    assert dev["grad_norm"] <= 1e-4 and dev["grad_proj"] <= 1e-4, dev


# ---------------------------------------------------------------------------------------------- 5. one update
def _teacher_rollout(T):
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    from settlers_of_catan_rl_amd.rollout import RolloutCollector
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy
    torch.manual_seed(0)
    env = _env(N, SEED)
    env.random_rollout(0, 300)
    net = CatanPolicy().cuda()
    return net, RolloutCollector(env, net, T, seed=1, teacher=ScriptedPolicy(env)).gather_rollouts()


def test_update_with_the_imitation_term(hip_lib, monkeypatch):
    """T = 8, N = 64, one epoch of two minibatches, teacher_coef = 1, fp32: trainer.teacher is the fp64 read-out of the two steps' teacher
    log-probs, no row skipped.  With teacher_coef = 0 the update is the one of a storage without labels: no teacher launch, and the
    parameters are the parent path's.  On the device two runs of the PARENT path already differ in the last bits (the backward kernels add
    with fp32 atomics; tests/test_gpu_ppo_diag.py::test_turning_it_on_changes_nothing), so "equal" is measured as that test measures
    it - against the spread of two parent runs; tests/test_teacher_cpu.py has the bit-equality where the arithmetic is deterministic."""
    from settlers_of_catan_rl_amd import ppo
    from settlers_of_catan_rl_amd.rollout import RolloutStorage
    from settlers_of_catan_rl_amd.train import PPOTrainer, PPOConfig
    T = 8
    net0, st = _teacher_rollout(T)
    seen, real = [], ppo.imitation_loss

    def recording(lp, rows, block):
        seen.append((lp.detach().float().view(-1).cpu().numpy().copy(), rows[:, 0].cpu().numpy().copy()))
        return real(lp, rows, block)
    monkeypatch.setattr(ppo, "imitation_loss", recording)
    net = copy.deepcopy(net0)
    tr = PPOTrainer(net, PPOConfig(ppo_epoch=1, num_mini_batch=2, teacher_coef=1.0), autocast_dtype=None, seed=3)
    losses = tr.update(st)
    t = tr.teacher
    assert len(seen) == 2 and all(lp.size == T * N // 2 for lp, _ in seen) and all(np.isfinite(x) for x in losses)
    lp, typ = np.concatenate([s[0] for s in seen]), np.concatenate([s[1] for s in seen])
    assert np.isfinite(lp).all()
    nll = -lp.astype(np.float64)
    rows = T * N
    # a mean of k fp64 terms summed in any order, then one division: within (k + 2) * 2^-52 * sum|term| / k of the exactly rounded one
    tol = lambda a: (a.size + 2) * 2.0 ** -52 * float(np.abs(a).sum()) / max(1, a.size)
    assert t["rows"] == rows and t["steps"] == 2 and t["skipped"] == 0
    assert abs(t["nll"] - math.fsum(nll) / rows) <= tol(nll) and t["nll_max"] == float(nll.max())
    assert t["half_share"] == np.count_nonzero(lp > HALF) / rows
    assert t["rows_by_type"] == [int(np.count_nonzero(typ == k)) for k in range(13)]
    for k in range(13):
        sel = nll[typ == k]
        assert (math.isnan(t["nll_by_type"][k]) and sel.size == 0) or abs(t["nll_by_type"][k] - math.fsum(sel) / sel.size) <= tol(sel), k
    moved = max(float((a - b).abs().max()) for a, b in zip(net.parameters(), net0.parameters()))
    assert moved > 0
    # teacher_coef = 0: the parent path, labels or not
    plain = RolloutStorage(T, N, "cuda")
    for k in STORAGE_KEYS:
        setattr(plain, k, getattr(st, k))
    calls = []
    real_eval = type(net0).evaluate_actions

    def counting_eval(self, *a, **kw):
        calls.append(sorted(kw))
        return real_eval(self, *a, **kw)
    monkeypatch.setattr(type(net0), "evaluate_actions", counting_eval)
    res = []
    for storage, cfg in ((st, dict(teacher_coef=0.0)), (plain, dict()), (plain, dict())):
        n2 = copy.deepcopy(net0)
        tr2 = PPOTrainer(n2, PPOConfig(ppo_epoch=1, num_mini_batch=2, lr=5e-3, **cfg), autocast_dtype=None, seed=3)
        assert all(np.isfinite(x) for x in tr2.update(storage)) and tr2.teacher is None
        res.append(torch.cat([p.detach().reshape(-1) for p in n2.parameters()]))
    assert len(seen) == 2 and len(calls) == 6 and all("teacher_actions" not in c and "teacher_grouping" not in c for c in calls)   # the parent's calls, no further launch
    noise, diff = float((res[1] - res[2]).abs().max()), float((res[0] - res[1]).abs().max())
    moved = float((res[1] - torch.cat([p.detach().reshape(-1) for p in net0.parameters()])).abs().max())
    print("teacher_coef = 0 against the parent path:", diff, "parent against parent:", noise, "moved:", moved)
    assert moved > 1e-3 and diff <= 4.0 * noise + 1e-6, (diff, noise, moved)
    with pytest.raises(ValueError, match="teacher_actions"):
        PPOTrainer(copy.deepcopy(net0), PPOConfig(ppo_epoch=1, num_mini_batch=2, teacher_coef=1.0), autocast_dtype=None, seed=3).update(plain)
