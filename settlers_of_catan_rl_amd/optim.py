"""The optimiser step of `PPO.update` - `nn.utils.clip_grad_norm_(parameters, max_grad_norm)` followed by `optim.Adam(lr, eps).step()`
(reference RL/ppo/ppo.py:23,67-68) - as ONE call over all parameters.

On the device it is two launches of `catan_adam_step` (csrc/catan_optim.hip: per-chunk sums of squared gradients; norm, clip
coefficient and the Adam update per chunk) instead of clip_grad_norm_'s three and Adam's nine `_foreach_*` launches over ~300 tensors
(0.55 ms -> ~0.05 ms of a minibatch step).  The exponential averages live in two flat buffers, the gradients stay wherever autograd
(or the flat all-reduce bucket, dist.GradBucket) put them: only their addresses are handed over, through a pinned host array, each
step.  On the CPU the same update runs as torch operations (what the tests compare with torch.optim.Adam)."""
import ctypes as C

import numpy as np
import torch


class FusedAdam(object):
    """`torch.optim.Adam(params, lr, betas, eps)` (no weight decay, no amsgrad) + gradient-norm clipping in `step(max_grad_norm)`.
    `param_groups[0]["lr"]` is read at every step (train_loop's linear decay writes it, as RL/robust_train.py:67-72 does).

    A parameter whose `.grad` is None in a step: by default it takes no step and its own step count stays where it is (its later
    bias corrections use that count), as torch.optim.Adam.  With `none_grad_is_zero=True` it takes the step of a ZERO gradient
    instead (its moments decay, it keeps moving by momentum): what torch.optim.Adam does in PPO.update, where the reference's
    action heads give every parameter a gradient tensor in every minibatch (zero for a head no row of the minibatch uses,
    RL/models/action_heads_module.py: the masked log-prob and entropy are multiplied by 0), while this package's compact heads
    do not run a head without rows and leave its gradients None."""
    RING = 8

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, none_grad_is_zero=False):
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("FusedAdam needs at least one parameter")
        dev = self.params[0].device
        if any(p.device != dev or p.dtype != torch.float32 or not p.is_contiguous() for p in self.params):
            raise ValueError("FusedAdam: contiguous fp32 parameters on one device")
        self.param_groups = [{"params": self.params, "lr": float(lr), "betas": (float(betas[0]), float(betas[1])), "eps": float(eps)}]
        self.device, self.steps = dev, 0
        self.none_grad_is_zero = bool(none_grad_is_zero)
        self.param_steps = np.zeros(len(self.params), dtype=np.int64)        # per tensor: the steps it took (torch.optim.Adam's state["step"])
        # every tensor's slice of the flat state starts on a 16-byte boundary
        offs, total = [], 0
        for p in self.params:
            offs.append(total)
            total += (p.numel() + 3) & ~3
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        self._m = [self.exp_avg[o:o + p.numel()].view_as(p) for o, p in zip(offs, self.params)]
        self._v = [self.exp_avg_sq[o:o + p.numel()].view_as(p) for o, p in zip(offs, self.params)]
        self.last_norm = None
        self._tables = None
        self.copied_grads = 0            # gradients that went through a temporary aligned fp32 copy (expected 0: tests / diagnostics)

    # ---- the device tables (built once; rebuilt if a parameter's storage moved)
    def _build_tables(self):
        from . import _lib
        L = _lib.lib()
        CH = int(L.catan_adam_chunk_elements())
        tens = np.zeros((len(self.params), 3), dtype=np.uint64)
        chunks = []
        for i, (p, m, v) in enumerate(zip(self.params, self._m, self._v)):
            if p.data_ptr() % 16:
                raise ValueError("FusedAdam: a parameter is not 16-byte aligned")
            tens[i] = (p.data_ptr(), m.data_ptr(), v.data_ptr())
            for o in range(0, p.numel(), CH):
                chunks.append((i, min(CH, p.numel() - o), o))
        ch = np.zeros(len(chunks), dtype=np.dtype([("tensor", np.int32), ("count", np.int32), ("offset", np.int64)]))
        for k, c in enumerate(chunks):
            ch[k] = c
        dev = self.device
        self._tables = {
            "sig": tuple(p.data_ptr() for p in self.params),
            "tensors": torch.from_numpy(tens.view(np.uint8).reshape(-1)).to(dev),
            "chunks": torch.from_numpy(ch.view(np.uint8).reshape(-1).copy()).to(dev), "n_chunks": len(chunks),
            # this step's gradient addresses travel through a RING of pinned host rows (the host runs several steps ahead of the device: one
            # row would be rewritten for step k + 1 before the copy engine has read step k's - the kernel would then take step k + 1's
            # gradient buffers, not yet written: round 5, found as NaN losses in the third update of bench.py) - a row is reused only
            # after the event recorded behind its copy has completed
            # a row: the n gradient addresses, then n pairs of fp32 (bias_correction1, bias_correction2_sqrt), one pair per tensor
            "grads_host": torch.zeros((self.RING, 2 * len(self.params)), dtype=torch.int64).pin_memory(),
            "grads": torch.zeros((self.RING, 2 * len(self.params)), dtype=torch.int64, device=dev),
            "grads_host_np": None,
            "events": [None] * self.RING, "slot": 0,
            "partial": torch.zeros(len(chunks), dtype=torch.float64, device=dev),
            "norm": torch.zeros(1, dtype=torch.float32, device=dev),
        }

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    @torch.no_grad()
    def step(self, max_grad_norm=None):
        """clip_grad_norm_(max_grad_norm) (None / <= 0: no clipping) + Adam.  The gradient tensors are read, not modified (torch's
        clip scales them in place; nothing reads them after the step).  -> None; `last_norm` holds the norm (a device scalar)."""
        g = self.param_groups[0]
        lr, (b1, b2), eps = float(g["lr"]), g["betas"], float(g["eps"])
        self.steps += 1
        has = np.fromiter((p.grad is not None for p in self.params), dtype=bool, count=len(self.params))
        stepped = np.ones_like(has) if self.none_grad_is_zero else has
        self.param_steps += stepped
        # the bias corrections of every tensor's own step count (in double, as torch does on the host; a tensor that never stepped
        # gets those of step 1 - it is not updated)
        t = np.maximum(self.param_steps, 1).astype(np.float64)
        bc1 = 1.0 - np.power(float(b1), t)
        bc2_sqrt = np.sqrt(1.0 - np.power(float(b2), t))
        clip = float(max_grad_norm) if (max_grad_norm is not None and max_grad_norm > 0) else 0.0
        if self.device.type != "cuda":
            return self._step_torch(lr, b1, b2, eps, bc1, bc2_sqrt, clip)
        from . import _lib
        if self._tables is None or self._tables["sig"] != tuple(p.data_ptr() for p in self.params):
            self._build_tables()
        t = self._tables
        n = len(self.params)
        if t["grads_host_np"] is None:
            t["grads_host_np"] = t["grads_host"].numpy()      # shares the pinned memory
            t["bias_host_np"] = t["grads_host_np"][:, n:].view(np.float32).reshape(self.RING, n, 2)
        k = t["slot"] = (t["slot"] + 1) % self.RING
        if t["events"][k] is not None:
            t["events"][k].synchronize()                      # the copy (and the step) that last used this row is done
        ptrs, keep = [], []
        for p in self.params:
            gr = p.grad
            if gr is None:
                ptrs.append(0)
                continue
            if gr.dtype != torch.float32 or not gr.is_contiguous() or gr.data_ptr() % 16:
                # the kernels read 16-byte vectors of fp32: anything else goes through a temporary copy.  p.grad itself is never replaced
                # (it may be a view of dist.GradBucket's flat buffer - whose views are 16-byte aligned, so that path does not come here)
                gr = gr.float().contiguous().clone()
                keep.append(gr)          # (freed after the launch is queued: the caching allocator keeps it valid for this stream's kernels)
                self.copied_grads += 1
            ptrs.append(gr.data_ptr())
        t["grads_host_np"][k, :n] = ptrs                      # (numpy assignments: element-wise writes into the tensor were ~300 aten ops per step)
        t["bias_host_np"][k, :, 0] = bc1
        t["bias_host_np"][k, :, 1] = bc2_sqrt
        host = t["grads_host"][k]
        t["grads"][k].copy_(host, non_blocking=True)
        P = lambda x: C.c_void_p(x.data_ptr())
        _lib.check(_lib.lib().catan_adam_step(P(t["tensors"]), P(t["chunks"]), t["n_chunks"], P(t["grads"][k]), n, int(self.none_grad_is_zero),
                                              P(t["partial"]), clip, lr, b1, b2, eps, P(t["norm"]), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        if t["events"][k] is None:
            t["events"][k] = torch.cuda.Event()
        t["events"][k].record()
        self.last_norm = t["norm"]
        # the kernel wrote the parameters behind autograd's back: bump the version counters of every parameter it stepped, as an
        # in-place torch update would (caches of derived data are keyed on them: nn_kernels.tile_encoder_pack, weight_images, an
        # inference copy's refresh)
        torch.autograd.graph.increment_version([p for p, s in zip(self.params, stepped) if s])

    def _step_torch(self, lr, b1, b2, eps, bc1, bc2_sqrt, clip):
        grads = [(p, m, v, p.grad, i) for i, (p, m, v) in enumerate(zip(self.params, self._m, self._v))
                 if p.grad is not None or self.none_grad_is_zero]
        if not grads:
            return
        present = [gr for _, _, _, gr, _ in grads if gr is not None]
        total = torch.sqrt(sum((gr.double() ** 2).sum() for gr in present)).float() if present else torch.zeros(())
        coef = torch.clamp(clip / (total + 1e-6), max=1.0) if clip > 0 else torch.ones(())
        for p, m, v, gr, i in grads:
            gc = gr * coef if gr is not None else torch.zeros_like(p)
            m.lerp_(gc, 1.0 - b1)
            v.mul_(b2).addcmul_(gc, gc, value=1.0 - b2)
            p.addcdiv_(m, (v.sqrt() / float(bc2_sqrt[i])).add_(eps), value=-(lr / float(bc1[i])))
        self.last_norm = total.reshape(1)

    # ---- checkpoints (torch.optim.Adam's layout: state per parameter index, each with its own step count)
    def state_dict(self):
        return {"state": {i: {"step": torch.tensor(float(self.param_steps[i])), "exp_avg": m.detach().clone(), "exp_avg_sq": v.detach().clone()}
                          for i, (m, v) in enumerate(zip(self._m, self._v))},
                "param_groups": [{k: v for k, v in self.param_groups[0].items() if k != "params"} | {"params": list(range(len(self.params)))}]}

    def load_state_dict(self, sd):
        # per-parameter step counts (they differ where a parameter had no gradient in some steps); a parameter without an entry (torch
        # keeps no state for a parameter that never stepped) starts from zero.  `steps`, the optimiser's own count, is the largest.
        # Refuse a parameter list that is not this optimiser's instead of loading something subtly different
        n_saved = len(sd["param_groups"][0]["params"]) if sd.get("param_groups") else len(sd["state"])
        idx = [int(i) for i in sd["state"]]
        if n_saved != len(self.params) or any(i < 0 or i >= len(self.params) for i in idx):
            raise ValueError(f"FusedAdam.load_state_dict: a state of {n_saved} parameters for {len(self.params)} parameters")
        for i, s in sd["state"].items():
            if tuple(s["exp_avg"].shape) != tuple(self._m[int(i)].shape):
                raise ValueError(f"FusedAdam.load_state_dict: state {i} has shape {tuple(s['exp_avg'].shape)}, the parameter {tuple(self._m[int(i)].shape)}")
        self.exp_avg.zero_(); self.exp_avg_sq.zero_()
        self.param_steps[:] = 0
        for i, s in sd["state"].items():
            self._m[int(i)].copy_(s["exp_avg"]); self._v[int(i)].copy_(s["exp_avg_sq"])
            self.param_steps[int(i)] = int(float(s["step"]))
        self.steps = int(self.param_steps.max()) if len(self.params) else 0
        for k in ("lr", "betas", "eps"):
            if k in sd["param_groups"][0]:
                self.param_groups[0][k] = sd["param_groups"][0][k]
