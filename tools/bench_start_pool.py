"""What the start pool costs a step: catan_step and catan_step_deferred in microseconds per call at 65 536 games with no pool
installed, and with a 4 096-entry pool at fresh_share 0 and 0.5; and the time of catan_start_pool_set itself.  Three runs each, every run
a fresh process; the configurations alternate inside a round and their order rotates from round to round, so that drift of the machine
hits them alike.

usage: bench_start_pool.py [--games N] [--calls K] [--warmup W] [--runs R] [--entries M] [--parent-library libcatan_hip.so] [--off-only]
                           [--out profiles/start_pool_bench.txt]

--parent-library: a libcatan_hip.so built from the parent commit; its off-path (the only one it has) runs as one more configuration in
every round.  The off case of this commit passes if its mean lies inside the spread (min..max) of the parent's runs (or below it).
A call is: the uniform-random sampler (catan_sample_random_actions), then the step - the same in every configuration.  Timed with the
host clock around K calls that end in a device synchronise.  The pool's entries are the unfinished states of the first M games after
600 random steps, so an installed game is a mid-game position; the counts of a run's deals are reported beside its times."""
import argparse
import json
import os
import time

import parent_compare as pc


def child(a):
    pc.use_library(a.library)                       # the parent commit's library under this commit's Python (the off-path uses nothing new)
    import torch
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    env = VecCatanEnv(a.games, seed=1)
    out = {"entries": a.entries, "fresh": a.fresh, "library": a.library or "this commit"}
    if a.entries:
        from settlers_of_catan_rl_amd.start_pool import StartPool
        src = VecCatanEnv(a.games, seed=2)
        src.random_rollout(0, 600)
        blobs = torch.from_numpy(StartPool.from_env(src, games=range(min(a.games, 2 * a.entries))).blobs[:a.entries]).to(env.device)
        assert blobs.shape[0] == a.entries, blobs.shape
        del src
        sets = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.set_start_pool(blobs, a.fresh)          # (ends in a stream synchronise of its own: the finished-position check)
            sets.append((time.perf_counter() - t0) * 1e6)
        out["set_us"] = sets

    def between(name, phase):                       # the deals of the timed calls alone
        c = env.start_pool_counts(reset=True)
        if phase == "timed":
            out[name + "_deals"] = [c["pool"], c["fresh"]]
    out.update(pc.step_call_times(env, a.calls, a.warmup, between if a.entries else None))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--entries", type=int, default=4096)
    ap.add_argument("--parent-library")
    ap.add_argument("--out", default=os.path.join(pc.ROOT, "profiles", "start_pool_bench.txt"))
    ap.add_argument("--off-only", action="store_true", help="only the configurations without a pool (the comparison with the parent)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--fresh", type=float, default=0.0)
    ap.add_argument("--library")
    a = ap.parse_args()
    if a.child:
        return child(a)
    configs = [("off", 0, 0.0, None), (f"{a.entries} entries, fresh 0", a.entries, 0.0, None), (f"{a.entries} entries, fresh 0.5", a.entries, 0.5, None)]
    if a.parent_library:
        configs.insert(0, ("parent, off", 0, 0.0, a.parent_library))
    if a.off_only:
        configs = [c for c in configs if c[1] == 0]
    rows = {c[0]: [] for c in configs}
    for r in range(a.runs):
        for label, entries, fresh, lib in pc.order(configs, r, "rotate"):  # (no configuration always runs behind the same neighbour)
            res = pc.run_child(__file__, ["--child", "--games", str(a.games), "--calls", str(a.calls), "--warmup", str(a.warmup), "--entries", str(entries),
                                          "--fresh", str(fresh)] + (["--library", lib] if lib else []), 300, "RESULT ")
            rows[label].append(res)
            print(f"run {r} {label:26s} {json.dumps(res)}", flush=True)
    lines = ["Start pool: what a pool costs a step (tools/bench_start_pool.py)",
             f"commit {pc.commit_of_tree()}; {a.games} games, {a.calls} timed calls behind {a.warmup} warm-up calls, {a.runs} runs each,",
             "a fresh process per run, configurations alternating; a call = catan_sample_random_actions + the step; host clock around the calls,",
             "ending in a device synchronise.  Microseconds per call.", ""]
    for key in ("catan_step_us", "catan_step_deferred_us"):
        lines.append(key[:-3])
        for label, _, _, _ in configs:
            v = [x[key] for x in rows[label]]
            lines.append(f"  {label:26s} runs {' '.join(f'{x:8.2f}' for x in v)}   mean {sum(v) / len(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}")
        if a.parent_library:
            lines.append("  off against the parent: " + pc.sentence([x[key] for x in rows["off"]], [x[key] for x in rows["parent, off"]], False))
        lines.append("")
    for label, entries, _, _ in configs:
        if entries:
            first = rows[label][0]
            sets = [s for x in rows[label] for s in x["set_us"][1:]]
            lines.append(f"{label}: deals in the timed calls of a run (pool, fresh): catan_step {first['catan_step_deals']}, "
                         f"catan_step_deferred {first['catan_step_deferred_deals']}")
            lines.append(f"  catan_start_pool_set of {entries} entries (blobs on the device; the first call of a process left out): "
                         f"mean {sum(sets) / len(sets):.1f} us, min {min(sets):.1f}, max {max(sets):.1f} over {len(sets)} calls;"
                         " first calls " + " ".join("%.0f" % x["set_us"][0] for x in rows[label]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
