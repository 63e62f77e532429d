"""GAE and clipped-PPO loss on the HIP kernels (csrc/catan_ppo.hip), mirroring the reference's
BatchProcessor.compute_advantages_alt (RL/ppo/process_batch.py:134-142) and PPO.update loss (RL/ppo/ppo.py:46-66).
torch is plumbing: device buffers, streams, autograd hookup and (for N>1 ranks) the 3-scalar all-reduce."""
import ctypes as C

import torch

from . import _lib


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _hip_gae_raw(r, v, m, gamma, gae_lambda):
    """k_gae + k_adv_stats: -> (returns, adv_raw, stats3 = (sum, sum of squares, count) of adv_raw as float64[3])"""
    L = _lib.lib()
    T, N = r.shape
    returns = torch.empty_like(r)
    adv = torch.empty_like(r)
    ws = torch.empty((L.catan_gae_workspace_doubles(N),), dtype=torch.float64, device=r.device)
    stats = torch.empty((3,), dtype=torch.float64, device=r.device)
    _lib.check(L.catan_gae(_ptr(r), _ptr(v), _ptr(m), T, N, float(gamma), float(gae_lambda), _ptr(returns), _ptr(adv),
                           _ptr(ws), _ptr(stats), _stream()))
    return returns, adv, stats


def _hip_adv_normalise(adv, stats):
    """k_adv_normalise, in place"""
    _lib.check(_lib.lib().catan_adv_normalise(_ptr(adv), adv.numel(), _ptr(stats), _stream()))
    return adv


# the two device back-ends of compute_gae; the world_size-2 gloo test swaps in torch stand-ins so that the function's own
# distributed logic (what is reduced, over which group, in which order) runs on CPU
_gae_raw, _adv_normalise = _hip_gae_raw, _hip_adv_normalise


def compute_gae(rewards, values, masks, gamma=0.999, gae_lambda=0.95, process_group=None, normalise=True):
    """rewards [T,N], values [T+1,N] (denormalised), masks [T+1,N] float32 CUDA -> (returns [T,N], advantages [T,N]).
    When torch.distributed is initialised the advantage mean/std are global over all ranks (three doubles
    all-reduced over `process_group`, default group if None); pass process_group=False to keep them rank-local."""
    T, N = rewards.shape
    assert values.shape == (T + 1, N) and masks.shape == (T + 1, N)
    r, v, m = (x.contiguous().float() for x in (rewards, values, masks))
    returns, adv, stats = _gae_raw(r, v, m, gamma, gae_lambda)
    if normalise:
        dist = torch.distributed
        if process_group is not False and dist.is_available() and dist.is_initialized() and dist.get_world_size(process_group) > 1:
            dist.all_reduce(stats, group=process_group)     # (sum, sumsq, count) over all ranks: global mean / std
        adv = _adv_normalise(adv, stats)
    return returns, adv


_LOSS_WS = {}


def _loss_workspace(device):
    """zeroed once; every k_ppo_loss call leaves it zero (include/catan_hip.h).  One per (device, STREAM): launches in flight on
    two streams (the trainer beside the reference_api.PPO adapter, a side-stream caller) must not share partial sums and the
    arrival counter."""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0)
    if key not in _LOSS_WS:
        _LOSS_WS[key] = torch.zeros((_lib.lib().catan_ppo_loss_workspace_doubles(),), dtype=torch.float64, device=device)
    return _LOSS_WS[key]


class _PpoLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp, values, old_logp, adv, old_values, returns, clip, value_coef, norm):
        L = _lib.lib()
        B = logp.numel()
        args = [x.contiguous().float().view(-1) for x in (logp, old_logp, adv, values, old_values, returns)]
        losses = torch.empty((2,), dtype=torch.float32, device=logp.device)
        d_logp = torch.empty((B,), dtype=torch.float32, device=logp.device)
        d_values = torch.empty((B,), dtype=torch.float32, device=logp.device)
        use_norm, mean, std = (0, 0.0, 1.0) if norm is None else (1, float(norm[0]), float(norm[1]))
        _lib.check(L.catan_ppo_loss(*[_ptr(x) for x in args], B, float(clip), float(value_coef), use_norm, mean, std,
                                    _ptr(losses), _ptr(d_logp), _ptr(d_values), _ptr(_loss_workspace(logp.device)), _stream()))
        ctx.save_for_backward(d_logp, d_values)
        ctx.shapes = (logp.shape, values.shape)
        total = losses[1] * value_coef + losses[0]
        ctx.mark_non_differentiable(losses)
        return total, losses

    @staticmethod
    def backward(ctx, g_total, _g_losses):
        d_logp, d_values = ctx.saved_tensors
        return (g_total * d_logp).view(ctx.shapes[0]), (g_total * d_values).view(ctx.shapes[1]), None, None, None, None, None, None, None


def _hip_ppo_loss(action_log_probs, values, old_action_log_probs, adv_targets, value_preds, returns, clip_param, value_loss_coef,
                  value_normaliser):
    return _PpoLoss.apply(action_log_probs, values, old_action_log_probs, adv_targets, value_preds, returns,
                          clip_param, value_loss_coef, value_normaliser)


_loss_backend = _hip_ppo_loss        # (replaceable like the GAE back-ends above)


def ppo_loss(action_log_probs, values, old_action_log_probs, adv_targets, value_preds, returns, clip_param=0.2,
             value_loss_coef=1.0, value_normaliser=None):
    """-> (value_loss_coef * value_loss + action_loss, (action_loss, value_loss)).  `value_normaliser` = (mean, std)
    applies RL/models/utils.py:17-18 to value_preds and returns first, as RL/ppo/ppo.py:46-48 does."""
    return _loss_backend(action_log_probs, values, old_action_log_probs, adv_targets, value_preds, returns,
                         clip_param, value_loss_coef, value_normaliser)


# ------------------------------------------------------------------------------------------------ update diagnostics
# What the clipped objective did during an update (k_ppo_diag, csrc/catan_ppo.hip; the words are listed in include/catan_hip_nn.h
# and DESIGN.md 8.7): accumulated on the device into one block of DIAG_WORDS doubles per epoch, read by the host once per update.
DIAG_WORDS = 20
DIAG_MAX_WORDS = (4, 5, 19)                                                        # maxima over calls (and over ranks)
DIAG_PER_STEP_WORDS = (1, 16, 17, 18)        # the same on every rank (steps, and the step's global scalars): a sum over ranks / world size

_DIAG_WS = {}


def _diag_workspace(device):
    """zeroed once; every k_ppo_diag call leaves it all zero (include/catan_hip_nn.h).  One per (device, STREAM), as _loss_workspace."""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0)
    if key not in _DIAG_WS:
        _DIAG_WS[key] = torch.zeros((_lib.lib().catan_ppo_diag_workspace_doubles(),), dtype=torch.float64, device=device)
    return _DIAG_WS[key]


def _check_diag_block(block):
    if block.dtype != torch.float64 or block.numel() != DIAG_WORDS or not block.is_contiguous():
        raise ValueError("ppo_diag: the block is a contiguous float64 tensor of %d words" % DIAG_WORDS)


def _scalar(x, device):
    if x is None:
        return None
    x = x.detach().float().reshape(-1)
    if x.numel() != 1 or x.device != device:
        raise ValueError("ppo_diag: entropy / grad_norm are one-element tensors on the rows' device")
    return x


def _hip_ppo_diag(block, logp, values, old_logp, adv, old_values, returns, clip, norm, entropy, grad_norm, max_grad_norm):
    """k_ppo_diag on the current stream (all calls into one block must come from one stream)"""
    _check_diag_block(block)
    if not block.is_cuda or block.device != logp.device:
        raise ValueError("ppo_diag: the block lives on the rows' device")
    args = [x.detach().contiguous().float().view(-1) for x in (logp, old_logp, adv, values, old_values, returns)]
    ent, gn = _scalar(entropy, logp.device), _scalar(grad_norm, logp.device)
    use_norm, mean, std = (0, 0.0, 1.0) if norm is None else (1, float(norm[0]), float(norm[1]))
    _lib.check(_lib.lib().catan_ppo_diag(*[_ptr(x) for x in args], args[0].numel(), float(clip), use_norm, mean, std,
                                         None if ent is None else _ptr(ent), None if gn is None else _ptr(gn), float(max_grad_norm),
                                         _ptr(block), _ptr(_diag_workspace(logp.device)), _stream()))


def _torch_ppo_diag(block, logp, values, old_logp, adv, old_values, returns, clip, norm, entropy, grad_norm, max_grad_norm):
    """The same twenty words as torch operations (tensors that are not on the device: the CPU tests, a CPU learner): the decisions of
    words 6..9 in fp32 as the loss takes them, the sums in fp64."""
    _check_diag_block(block)
    f32 = torch.float32
    lp, ol, ad, v, vp0, ret0 = (x.detach().reshape(-1).to(f32) for x in (logp, old_logp, adv, values, old_values, returns))
    clip32 = torch.tensor(float(clip), dtype=f32)
    vp, ret = vp0, ret0
    if norm is not None:
        mean32, den32 = torch.tensor(float(norm[0]), dtype=f32), torch.tensor(float(norm[1]), dtype=f32) + torch.tensor(1e-4, dtype=f32)
        vp, ret = (vp0 - mean32) / den32, (ret0 - mean32) / den32
    lo, hi = 1.0 - clip32, 1.0 + clip32
    ratio = torch.exp(lp - ol)
    s1, s2 = ratio * ad, torch.minimum(torch.maximum(ratio, lo), hi) * ad
    inside = (ratio >= lo) & (ratio <= hi)
    dv = v - vp
    vc = vp + torch.minimum(torch.maximum(dv, -clip32), clip32)
    l1, l2 = (v - ret) ** 2, (vc - ret) ** 2
    vin = (dv >= -clip32) & (dv <= clip32)
    d = lp.double() - ol.double()
    vpd, rd = vp0.double(), ret0.double()
    if norm is not None:
        mean, den = float(mean32), float(torch.tensor(float(norm[1]), dtype=f32)) + 1e-4
        vpd, rd = (vpd - mean) / den, (rd - mean) / den
    e, e0 = rd - v.double(), rd - vpd
    zero = torch.zeros((), dtype=torch.float64)
    w = [zero] * DIAG_WORDS
    w[0], w[1] = zero + float(lp.numel()), zero + 1.0
    w[2], w[3] = (-d).sum(), (torch.expm1(d) - d).sum()
    w[4], w[5] = torch.clamp(d, min=0.0).max(), torch.clamp(-d, min=0.0).max()
    w[6], w[7] = (~inside).sum().double(), (~inside & (s1 > s2)).sum().double()
    w[8], w[9] = (~vin).sum().double(), (~(l1 >= l2) & ~vin).sum().double()
    w[10], w[11], w[12], w[13], w[14], w[15] = rd.sum(), (rd * rd).sum(), e.sum(), (e * e).sum(), e0.sum(), (e0 * e0).sum()
    ent, gn = _scalar(entropy, lp.device), _scalar(grad_norm, lp.device)
    touched = set(range(16))
    if ent is not None:
        w[16] = ent[0].double()
        touched.add(16)
    if gn is not None:
        w[17], w[19] = gn[0].double(), gn[0].double()
        w[18] = ((gn[0] > torch.tensor(float(max_grad_norm), dtype=f32)) & (float(max_grad_norm) > 0.0)).double()
        touched.update((17, 18, 19))
    new = torch.stack([x.to(block.device) for x in w]).reshape(block.shape)
    is_max = torch.zeros(DIAG_WORDS, dtype=torch.bool, device=block.device)
    is_max[list(DIAG_MAX_WORDS)] = True
    keep = torch.ones(DIAG_WORDS, dtype=torch.bool, device=block.device)
    keep[sorted(touched)] = False
    block.copy_(torch.where(keep.reshape(block.shape), block, torch.where(is_max.reshape(block.shape), torch.maximum(block, new), block + new)))


def _default_ppo_diag(block, logp, values, old_logp, adv, old_values, returns, clip, norm, entropy, grad_norm, max_grad_norm):
    backend = _hip_ppo_diag if logp.is_cuda else _torch_ppo_diag       # (rows on the device and no library: an error, not the torch form)
    return backend(block, logp, values, old_logp, adv, old_values, returns, clip, norm, entropy, grad_norm, max_grad_norm)


_diag_backend = _default_ppo_diag    # (replaceable like _loss_backend)


def ppo_diag(block, logp, values, old_logp, adv, old_values, returns, clip=0.2, value_normaliser=None, entropy=None, grad_norm=None,
             max_grad_norm=0.0):
    """One optimiser step's diagnostics, ADDED into `block` (float64 [20] on the rows' device, zeroed by the caller, one per epoch; all
    calls into one block on one stream).  The first six row arguments and `clip`, `value_normaliser` are ppo_loss's; `entropy`,
    `grad_norm`: one-element tensors of the step (or None: their words stay as they are).  No host read; `diag_summary` turns the
    blocks of an update into numbers once they are on the host."""
    _diag_backend(block, logp, values, old_logp, adv, old_values, returns, clip, value_normaliser, entropy, grad_norm, max_grad_norm)


def _diag_numbers(w):
    nan = float("nan")
    rows, steps = float(w[0]), float(w[1])
    per_row = (lambda x: float(x) / rows) if rows > 0 else (lambda x: nan)
    per_step = (lambda x: float(x) / steps) if steps > 0 else (lambda x: nan)

    def explained(s, ss):
        if not rows > 0:
            return nan
        var_ret = float(w[11]) / rows - (float(w[10]) / rows) ** 2
        if not var_ret > 0.0:
            return nan
        return 1.0 - (float(ss) / rows - (float(s) / rows) ** 2) / var_ret
    return {"approx_kl": per_row(w[3]), "approx_kl_k1": per_row(w[2]), "max_log_ratio_up": float(w[4]), "max_log_ratio_down": float(w[5]),
            "clip_fraction": per_row(w[6]), "policy_grad_zero_fraction": per_row(w[7]),
            "value_clip_fraction": per_row(w[8]), "value_grad_zero_fraction": per_row(w[9]),
            "explained_variance": explained(w[12], w[13]), "explained_variance_old": explained(w[14], w[15]),
            "entropy": per_step(w[16]), "grad_norm_mean": per_step(w[17]), "grad_norm_max": float(w[19]),
            "grad_clipped_fraction": per_step(w[18]), "rows": int(round(rows)), "steps": int(round(steps))}


def diag_summary(blocks):
    """blocks: HOST array [epochs][20] (the device blocks of an update, copied once) -> {key: [value per epoch], ...,
    "update": {key: value over all epochs}}.  approx_kl = word 3 / rows (the k3 estimator E[(r - 1) - log r]), approx_kl_k1 = word 2 /
    rows; the fractions are per row; explained_variance(_old) = 1 - Var(ret - v) / Var(ret) (v: the values being trained / the
    epoch's re-evaluated predictions), NaN when Var(ret) is 0; entropy, grad_norm_mean and grad_clipped_fraction are per step."""
    import numpy as np
    b = np.asarray(blocks, dtype=np.float64).reshape(-1, DIAG_WORDS)
    per = [_diag_numbers(row) for row in b]
    out = {k: [p[k] for p in per] for k in _diag_numbers(np.zeros(DIAG_WORDS))}
    total = b.sum(axis=0)
    for k in DIAG_MAX_WORDS:
        total[k] = b[:, k].max() if len(b) else 0.0
    out["update"] = _diag_numbers(total)
    return out


def reduce_diag_over_ranks(block):
    """In place, a device (or CPU, under gloo) tensor [..., 20] of blocks: two all-reduces over the default group - SUM, and MAX for
    the maximum words - then the words that are the same on every rank (steps, entropy and gradient-norm sums, clipped steps: every
    rank takes the same steps and the gradient norm is already global) divided by the world size.  Nothing without >1 rank."""
    dist = torch.distributed
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return block
    mx = block[..., list(DIAG_MAX_WORDS)].contiguous()
    dist.all_reduce(block, op=dist.ReduceOp.SUM)
    dist.all_reduce(mx, op=dist.ReduceOp.MAX)
    block[..., list(DIAG_MAX_WORDS)] = mx
    block[..., list(DIAG_PER_STEP_WORDS)] /= dist.get_world_size()
    return block


# ------------------------------------------------------------------------------------------------ imitation term (kickstarting)
# The teacher's rows under the net (k_imitation_loss, csrc/catan_players.hip; the words are listed in
# include/catan_hip_nn.h): the loss -mean(lp), its gradient and the read-out from ONE launch, accumulated like the diagnostics.
IMIT_WORDS = 33
IMIT_MAX_WORDS = (3,)
IMIT_PER_STEP_WORDS = (1,)               # the same on every rank (calls)
IMIT_HALF = -0.6931472                   # lp above this (as fp32): more than half the mass on the teacher's whole composite action

_IMIT_WS = {}


def _imit_workspace(device):
    """zeroed once; every k_imitation_loss call leaves it all zero.  One per (device, STREAM), as _loss_workspace."""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    if key not in _IMIT_WS:
        _IMIT_WS[key] = torch.zeros((_lib.lib().catan_imitation_loss_workspace_doubles(),), dtype=torch.float64, device=device)
    return _IMIT_WS[key]


def _check_imit(lp, teacher_rows, block):
    if block.dtype != torch.float64 or block.numel() != IMIT_WORDS or not block.is_contiguous() or block.device != lp.device:
        raise ValueError("imitation_loss: the block is a contiguous float64 tensor of %d words on the rows' device" % IMIT_WORDS)
    if teacher_rows.dim() != 2 or teacher_rows.shape[0] != lp.numel() or teacher_rows.shape[1] != 18 or lp.numel() < 1:
        raise ValueError("imitation_loss: lp [B] (B >= 1) and teacher_rows [B, 18]")


def _hip_imitation(lp, teacher_rows, block):
    """k_imitation_loss on the current stream -> (loss [1], dlp [B])"""
    x = lp.detach().contiguous().float().view(-1)
    rows = teacher_rows.contiguous() if teacher_rows.dtype == torch.int64 else teacher_rows.long().contiguous()
    loss = torch.empty((1,), dtype=torch.float32, device=x.device)
    dlp = torch.empty_like(x)
    _lib.check(_lib.lib().catan_imitation_loss(_ptr(x), _ptr(rows), x.numel(), _ptr(loss), _ptr(dlp), _ptr(block),
                                               _ptr(_imit_workspace(x.device)), _stream()))
    return loss, dlp


def _torch_imitation(lp, teacher_rows, block):
    """The same arithmetic as torch operations (tensors that are not on the device: the CPU tests, a CPU learner)."""
    x = lp.detach().reshape(-1).float()
    B = x.numel()
    finite = torch.isfinite(x)
    nll = torch.where(finite, -x.double(), torch.zeros((), dtype=torch.float64, device=x.device))
    typ = teacher_rows[:, 0].long()
    w = torch.zeros(IMIT_WORDS, dtype=torch.float64, device=x.device)
    w[0], w[1], w[2] = float(B), 1.0, nll.sum()
    w[4] = (finite & (x > torch.tensor(IMIT_HALF, dtype=torch.float32, device=x.device))).sum().double()
    w[5] = (~finite).sum().double()
    ok = finite & (typ >= 0) & (typ <= 12)
    w[6:19] = torch.bincount(typ[ok], minlength=13).double()
    w[19:32] = torch.zeros(13, dtype=torch.float64, device=x.device).index_add_(0, typ[ok], nll[ok])
    new = block + w.reshape(block.shape)
    new.view(-1)[3] = torch.maximum(block.view(-1)[3], nll.max())
    block.copy_(new)
    loss = (nll.sum() / B).float().reshape(1)
    dlp = torch.where(finite, torch.full_like(x, float(torch.tensor(-1.0 / B, dtype=torch.float64).float())), torch.zeros_like(x))
    return loss, dlp


class _Imitation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lp, teacher_rows, block):
        _check_imit(lp, teacher_rows, block)
        loss, dlp = (_hip_imitation if lp.is_cuda else _torch_imitation)(lp, teacher_rows, block)   # (rows on the device and no library: an error)
        ctx.save_for_backward(dlp)
        ctx.shape = lp.shape
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dlp,) = ctx.saved_tensors
        return (g * dlp).view(ctx.shape), None, None


def imitation_loss(lp, teacher_rows, block):
    """-> the scalar -mean(lp) over the rows whose lp is finite (divided by ALL B rows): the imitation term of a step, differentiable
    by lp (backward: g x dlp, dlp = -1 / B, 0 for a skipped row).  lp [B] or [B, 1]: the joint log-prob of the teacher's action rows
    (CatanPolicy.evaluate_actions(teacher_actions=...)); teacher_rows int64 [B, 18]; the step's read-out is ADDED into `block`
    (float64 [33] on the rows' device, zeroed by the caller; all calls into one block on one stream).  No host read;
    `imitation_summary` turns a block into numbers once it is on the host."""
    return _Imitation.apply(lp, teacher_rows, block)


def imitation_summary(block):
    """a HOST block [33] -> {"nll", "nll_max", "half_share" (rows with p > 1/2), "skipped", "rows", "steps", "rows_by_type" [13],
    "nll_by_type" [13] (NaN for a type without rows)}; the means are over the rows that were not skipped"""
    import numpy as np
    w = np.asarray(block, dtype=np.float64).reshape(IMIT_WORDS)
    nan = float("nan")
    rows, skipped = float(w[0]), float(w[5])
    used = rows - skipped
    return {"nll": float(w[2]) / used if used > 0 else nan, "nll_max": float(w[3]), "half_share": float(w[4]) / used if used > 0 else nan,
            "skipped": int(round(skipped)), "rows": int(round(rows)), "steps": int(round(float(w[1]))),
            "rows_by_type": [int(round(float(x))) for x in w[6:19]],
            "nll_by_type": [float(s) / float(c) if c > 0 else nan for s, c in zip(w[19:32], w[6:19])]}


def reduce_imitation_over_ranks(block):
    """In place, as reduce_diag_over_ranks: SUM over the default group, MAX for the maximum word, the call count divided by the world
    size.  Nothing without > 1 rank."""
    dist = torch.distributed
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return block
    mx = block[..., list(IMIT_MAX_WORDS)].contiguous()
    dist.all_reduce(block, op=dist.ReduceOp.SUM)
    dist.all_reduce(mx, op=dist.ReduceOp.MAX)
    block[..., list(IMIT_MAX_WORDS)] = mx
    block[..., list(IMIT_PER_STEP_WORDS)] /= dist.get_world_size()
    return block
