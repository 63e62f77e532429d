"""Times catan_state_fork against the path it replaces, on one stream with HIP events after a warm-up.

  (a) fork            catan_state_fork of roots x copies games, one call per search round
  (b) blob, round     the per-round edit of the draw-counter word (torch ops) + catan_state_import of roots x copies blobs
      blob, decision  catan_state_export of the roots + repeat_interleave to one blob per simulation, once per decision
at 4 096 roots x 16 copies and 65 536 x 1, and one ForwardSearch.act at config 5's shape under each `state_broadcast` setting.
The fraction of the HBM peak is on the algorithmic bytes of a copy: 704 B in once per distinct source + (704 + 44) B out per copy,
measured while rotating over source / destination sets larger together than the Infinity Cache; a cache-warm figure is printed beside it.

usage: python tools/bench_state_fork.py [--out profiles/state_fork_bench.txt] [--no-search]"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from settlers_of_catan_rl_amd import forward_search as fs, spec  # noqa: E402
from settlers_of_catan_rl_amd.env import VecCatanEnv  # noqa: E402

HBM_PEAK = 8.0e12


N_SETS = 5            # source / destination sets visited in turn: together > the 256 MiB Infinity Cache, so a call finds its data in HBM


def timed(fns, reps=20, warm=5):
    """fns: one callable per working set, called in turn -> (median, best) microseconds of a call"""
    for i in range(warm):
        fns[i % len(fns)]()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for i, (a, b) in enumerate(ev):
        a.record(); fns[i % len(fns)](); b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return ts[len(ts) // 2], ts[0]


def shape(roots, copies, lines):
    n = roots * copies
    src_idx = torch.arange(roots, device="cuda").repeat_interleave(copies)
    k = torch.arange(n, device="cuda") % copies
    stride = ((1 + k) << 22) & 0xFFFFFFFF
    w = spec.STATE_OFFSETS["rng_draws"][0]
    fork, blob, dec = [], [], []
    for i in range(N_SETS):
        src = VecCatanEnv(roots, seed=1 + i)
        src.random_rollout(0, 400)
        dst = VecCatanEnv(n, seed=100 + i, dense_reward=True, auto_reset=False)

        def decision(src=src):
            return src.export_state().repeat_interleave(copies, dim=0).clone()
        blobs = decision()
        base = blobs[:, w].long() & 0xFFFFFFFF

        def blob_round(dst=dst, blobs=blobs, base=base):
            sub = (base + stride) & 0xFFFFFFFF
            blobs[:, w] = torch.where(sub >= 2 ** 31, sub - 2 ** 32, sub).to(torch.int32)
            dst.import_state(blobs)
        fork.append(lambda dst=dst, src=src: dst.fork_from(src, src_idx, None, stride))
        blob.append(blob_round); dec.append(decision)
    algo = roots * 704 + n * (704 + 44)
    per_set = (roots * 704 + n * (704 + 128)) / 2 ** 20
    frac = lambda us: algo / (us * 1e-6) / HBM_PEAK * 100
    cold = {k_: timed(v) for k_, v in (("fork", fork), ("blob", blob), ("dec", dec))}
    warm = {k_: timed(v[:1]) for k_, v in (("fork", fork), ("blob", blob), ("dec", dec))}
    lines.append(f"{roots} roots x {copies} copies ({n} games, {algo} algorithmic bytes per fork): median (best) microseconds over 20 calls")
    lines.append(f"  rotating over {N_SETS} source/destination sets ({per_set:.0f} MiB of records and side rows each: the data of a call comes from HBM)")
    lines.append(f"    (a) catan_state_fork                           {cold['fork'][0]:9.1f} ({cold['fork'][1]:.1f})   {frac(cold['fork'][0]):.1f} % of the 8 TB/s HBM peak")
    lines.append(f"    (b) per round: blob edit + catan_state_import  {cold['blob'][0]:9.1f} ({cold['blob'][1]:.1f})")
    lines.append(f"        + once per decision, on top of every round's cost: export + repeat_interleave {cold['dec'][0]:9.1f} ({cold['dec'][1]:.1f})")
    lines.append("  one set over and over (cache-warm: the set stays in the Infinity Cache, this is NOT an HBM figure)")
    lines.append(f"    (a) {warm['fork'][0]:9.1f} ({warm['fork'][1]:.1f})   (b) per round {warm['blob'][0]:9.1f} ({warm['blob'][1]:.1f})   per decision {warm['dec'][0]:9.1f} ({warm['dec'][1]:.1f})")
    return cold["fork"][0], cold["blob"][0]


def search(mode, lines):
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    torch.manual_seed(0)
    R, S, K, D = 4096, 64, 16, 15
    root = VecCatanEnv(R, seed=0)
    root.random_rollout(0, 500)
    net = CatanPolicy().cuda().eval()
    s = fs.ForwardSearch(net, lambda n: VecCatanEnv(n, seed=1, env_id0=1 << 32, dense_reward=True, auto_reset=False), R, max_depth=D,
                         sims_per_root=S, sims_per_round=K, autocast_dtype=torch.bfloat16, use_graphs=True, state_broadcast=mode)
    s.act(root)                                                       # warm-up (graph captures)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    s.act(root)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    lines.append(f"  ForwardSearch.act, config 5 ({R} roots x {S} simulations, depth {D}), state_broadcast={mode!r}: {dt:.2f} s = {R * S / dt:,.0f} simulations/s")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_fork_bench.txt"))
    ap.add_argument("--no-search", action="store_true")
    args = ap.parse_args()
    lines = [f"tools/bench_state_fork.py on {torch.cuda.get_device_name(0)}; HIP events on one stream, warm-up first"]
    res = [shape(4096, 16, lines), shape(65536, 1, lines)]
    ok = all(a <= b for a, b in res)
    want = "fork" if ok else "blob"
    lines.append(f"fork not slower than the per-round blob path at both shapes: {ok} -> default state_broadcast {want!r} "
                 f"(forward_search.DEFAULT_STATE_BROADCAST is {fs.DEFAULT_STATE_BROADCAST!r})")
    if not args.no_search:
        for mode in ("fork", "blob"):
            search(mode, lines)
    import subprocess
    kr = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_fork", "k_masks_of_list"], stdout=subprocess.PIPE).stdout.decode()
    lines.append("tools/kernel_resources.py (registers, LDS, scratch of the new kernels):")
    lines += ["  " + x for x in kr.strip().splitlines()]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
