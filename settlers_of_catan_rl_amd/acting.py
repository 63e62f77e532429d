"""How the acting code (rollout collector, evaluation games, forward search) calls a policy net: `act`, the one eager call, and
`GraphedAct`, the same call captured per row-count bucket and replayed as a hipGraph."""
import torch


def act(net, args, autocast_dtype, **kw):
    """net.act(*args, **kw), under autocast where a dtype is given"""
    if autocast_dtype is None:
        return net.act(*args, **kw)
    with torch.autocast(device_type="cuda", dtype=autocast_dtype):
        return net.act(*args, **kw)


class GraphedAct(object):
    """policy.act for SMALL batches as hipGraph replays.  Towards the end of a round only a few simulations are still
    running, and a policy pass is then ~1 300 tiny kernels - launch-bound at ~10 ms whatever the batch.  For a few bucket
    sizes the pass is captured once (torch.cuda.CUDAGraph: the library GEMMs and the hand-written attention / LayerNorm
    launches alike, all on the capture stream) with static input buffers and replayed; rows beyond the live ones are
    padding and ignored.  Sampling uses torch's default CUDA generator, which graphs advance correctly.  Falls back to the
    eager call if capture is unavailable."""

    def __init__(self, policy, buckets=(512, 4096, 16384), autocast_dtype=None, deterministic=False, generator=None):
        """generator: the CUDA torch.Generator the sampling draws from (registered with every captured graph, so replays
        advance it as eager calls would); None = torch's default CUDA generator."""
        self.policy, self.buckets, self.autocast_dtype, self.deterministic = policy, tuple(sorted(buckets)), autocast_dtype, deterministic
        self.generator = generator
        self.graphs = {}
        self.failed = False

    def _run(self, f, lists, lens, masks):
        kw = {} if self.generator is None else {"generator": self.generator}
        return act(self.policy, (f, lists, lens, masks), self.autocast_dtype, deterministic=self.deterministic, **kw)

    def _capture(self, B, f, lists, lens, masks):
        st = {"f": f[:1].expand(B, -1).clone(), "lists": lists[:1].expand(B, -1, -1).clone(),
              "lens": lens[:1].expand(B, -1).clone(), "masks": masks[:1].expand(B, -1).clone()}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                self._run(st["f"], st["lists"], st["lens"], st["masks"])
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        if self.generator is not None:
            g.register_generator_state(self.generator)
        with torch.cuda.graph(g):
            v, a, lp = self._run(st["f"], st["lists"], st["lens"], st["masks"])[:3]
        st["g"], st["v"], st["a"], st["lp"] = g, v, a, lp
        st["sig"] = self._signature()
        return st

    def _signature(self):
        """where the policy's parameters live: a captured graph reads exactly these addresses"""
        ps = list(self.policy.parameters())
        return (len(ps), hash(tuple(p.data_ptr() for p in ps)), ps[0].dtype) if ps else ()   # EVERY parameter: one replaced in the middle is stale too

    def input_rows(self, B, n, obs_dtype):
        """May a producer write n rows straight into the input buffers of bucket B's captured graph (the env's catan_obs_rows / mask
        expansion: it saves the copy of every replay)?  -> the first n rows of (f, lists, lens, masks) if the bucket is captured and
        the buffers have the dtypes the producer writes (observations of obs_dtype, int32 lists and lens, float32 masks), else None."""
        st = self.graphs.get(B)
        if st is None or (st["f"].dtype, st["lists"].dtype, st["lens"].dtype, st["masks"].dtype) != (obs_dtype, torch.int32, torch.int32, torch.float32):
            return None
        return st["f"][:n], st["lists"][:n], st["lens"][:n], st["masks"][:n]

    def __call__(self, f, lists, lens, masks, with_logp=False, clone=True):
        """-> (value [n,1], actions [n,18]) (+ log-prob [n,1] with `with_logp`) for n rows; eager when n exceeds the largest
        bucket.  Inputs that ARE the graph's static buffers (input_rows) are not copied; clone=False hands out the graph's
        output buffers themselves (valid until the next replay)."""
        n = f.shape[0]
        B = next((b for b in self.buckets if n <= b), None)
        if B is None or self.failed or not f.is_cuda:
            v, a, lp = self._run(f, lists, lens, masks)[:3]
            return (v, a, lp) if with_logp else (v, a)
        if B not in self.graphs:
            try:
                self.graphs[B] = self._capture(B, f, lists, lens, masks)
            except Exception:                                   # capture not available: stay eager
                self.failed = True
                torch.cuda.synchronize()
                v, a, lp = self._run(f, lists, lens, masks)[:3]
                return (v, a, lp) if with_logp else (v, a)
        st = self.graphs[B]
        if st["sig"] != self._signature():                  # the parameters moved (a .to() / a rebuilt module): the graph is stale
            self.graphs.clear()
            return self.__call__(f, lists, lens, masks, with_logp)
        refresh = getattr(self.policy, "refresh_kernel_packs", None)
        if refresh is not None:
            refresh()                                           # host-side parameter packs a replay would not rebuild
        for k, x in (("f", f), ("lists", lists), ("lens", lens), ("masks", masks)):
            if x.data_ptr() != st[k].data_ptr():
                st[k][:n] = x
        st["g"].replay()
        out = (st["v"][:n], st["a"][:n], st["lp"][:n]) if with_logp else (st["v"][:n], st["a"][:n])
        return tuple(o.clone() for o in out) if clone else out
