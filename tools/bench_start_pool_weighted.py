"""What the start pool's weighted pick and outcome tallies cost: catan_step and catan_step_deferred in microseconds per call
at 65 536 games with no pool installed (the off-path, against the parent commit's library), with a uniform 4 096-entry pool, with the same
pool under weights, and under weights with the outcome tallies on; the time of catan_start_pool_set_weights itself; and bench.py with the
parent's library and this commit's in alternating pairs.  Three runs each, every run a fresh process; the configurations alternate inside
a round and their order rotates from round to round, so that drift of the machine hits them alike.

usage: bench_start_pool_weighted.py [--games N] [--calls K] [--warmup W] [--runs R] [--entries M] [--parent-library libcatan_hip.so]
                                    [--bench-runs B] [--out profiles/start_pool_weighted_bench.txt]

--parent-library: a libcatan_hip.so built from the parent commit; every configuration also runs under it, beside this commit's run in every
round (the on cases too: they need the parent's ABI to be this commit's), and bench.py runs under it in turn with this commit's.  A case
of this commit passes if its mean lies inside the spread (min..max) of the parent's runs (or on its better side).
A call is: the uniform-random sampler (catan_sample_random_actions), then the step - the same in every configuration.  Timed with the
host clock around K calls that end in a device synchronise.  The pool's entries are the unfinished states of the first M games after 600
random steps; the weights are M seeded values in 0..65 535, every eighth of them 0."""
import argparse
import json
import os
import time

import parent_compare as pc


def child(a):
    pc.use_library(a.library)
    import numpy as np
    import torch
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    env = VecCatanEnv(a.games, seed=1)
    out = {"mode": a.mode, "library": a.library or "this commit"}
    if a.mode != "off":
        from settlers_of_catan_rl_amd.start_pool import StartPool
        src = VecCatanEnv(a.games, seed=2)
        src.random_rollout(0, 600)
        blobs = torch.from_numpy(StartPool.from_env(src, games=range(min(a.games, 2 * a.entries))).blobs[:a.entries]).to(env.device)
        assert blobs.shape[0] == a.entries, blobs.shape
        del src
        env.set_start_pool(blobs, 0.0)
        if a.mode in ("weighted", "weighted+outcomes"):
            w = np.random.RandomState(7).randint(0, 65536, a.entries).astype(np.int64)
            w[::8] = 0
            times = []
            for _ in range(6):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                env.set_start_pool_weights(w)          # (host checks, the upload, the scan, one stream synchronise, the drain of the env's streams)
                times.append((time.perf_counter() - t0) * 1e6)
            out["set_weights_us"] = times
        if a.mode == "weighted+outcomes":
            env.enable_start_pool_outcomes(torch.arange(a.games, device=env.device) % 4 + 1)
        env.reset()

    def between(name, phase):                       # the deals and tallies of the timed calls alone
        c = env.start_pool_counts(reset=True)
        if phase == "timed":
            out[name + "_deals"] = [c["pool"], c["fresh"]]
            out[name + "_entries_hit"] = int((c["per_entry"] > 0).sum())
            if a.mode == "weighted+outcomes":
                o = env.start_pool_outcomes(reset=True)
                out[name + "_tallied"] = [o["seen"], o["skipped"]]
    out.update(pc.step_call_times(env, a.calls, a.warmup, between if a.mode != "off" else None))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--entries", type=int, default=4096)
    ap.add_argument("--parent-library")
    ap.add_argument("--bench-runs", type=int, default=3, help="pairs of bench.py runs (0: none)")
    ap.add_argument("--bench-steps", type=int, default=4096)
    ap.add_argument("--bench-warmup", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(pc.ROOT, "profiles", "start_pool_weighted_bench.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--bench-child", action="store_true")
    ap.add_argument("--mode", default="off", choices=["off", "uniform", "weighted", "weighted+outcomes"])
    ap.add_argument("--library")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.bench_child:
        return pc.bench_py_child(a.library, a.bench_steps, a.bench_warmup)
    configs = [("off", "off", None), (f"uniform, {a.entries} entries", "uniform", None), (f"weighted, {a.entries} entries", "weighted", None),
               ("weighted + outcomes", "weighted+outcomes", None)]
    if a.parent_library:
        configs = [c for label, mode, _ in configs for c in ((f"parent, {label}", mode, a.parent_library), (label, mode, None))]
    rows = {c[0]: [] for c in configs}
    for r in range(a.runs):
        for label, mode, lib in pc.order(configs, r, "rotate"):  # (no configuration always runs behind the same neighbour)
            res = pc.run_child(__file__, ["--child", "--games", str(a.games), "--calls", str(a.calls), "--warmup", str(a.warmup), "--entries", str(a.entries),
                                          "--mode", mode] + (["--library", lib] if lib else []), 300, "RESULT ")
            rows[label].append(res)
            print(f"run {r} {label:34s} {json.dumps(res)}", flush=True)
    bench = pc.bench_py_runs(a.parent_library, a.bench_runs, a.bench_steps, a.bench_warmup, __file__, how="fixed", timeout=900)
    lines = ["Start pool, weighted picks and outcome tallies: what they cost a step (tools/bench_start_pool_weighted.py)",
             f"commit {pc.commit_of_tree()}; {a.games} games, {a.calls} timed calls behind {a.warmup} warm-up calls, {a.runs} runs each,",
             "a fresh process per run, configurations alternating; a call = catan_sample_random_actions + the step; host clock around the calls,",
             "ending in a device synchronise.  Microseconds per call.", ""]
    for key in ("catan_step_us", "catan_step_deferred_us"):
        lines.append(key[:-3])
        for label, _, _ in configs:
            v = [x[key] for x in rows[label]]
            lines.append(f"  {label:34s} runs {' '.join(f'{x:8.2f}' for x in v)}   mean {sum(v) / len(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}")
        for label, _, lib in configs if a.parent_library else []:
            if lib:
                continue
            lines.append(f"  {label} against the parent: " + pc.sentence([x[key] for x in rows[label]], [x[key] for x in rows["parent, " + label]], False))
        lines.append("")
    for label, mode, _ in configs:
        if mode == "off":
            continue
        first = rows[label][0]
        lines.append(f"{label}: deals in the timed calls of a run (pool, fresh) and entries installed at least once: catan_step {first['catan_step_deals']} "
                     f"{first['catan_step_entries_hit']}, catan_step_deferred {first['catan_step_deferred_deals']} {first['catan_step_deferred_entries_hit']}")
        if "catan_step_tallied" in first:
            lines.append(f"  games tallied in the warm-up and the timed calls (seen, skipped): catan_step {first['catan_step_tallied']}, catan_step_deferred {first['catan_step_deferred_tallied']}")
        if "set_weights_us" in first:
            sets = [s for x in rows[label] for s in x["set_weights_us"][1:]]
            lines.append(f"  set_start_pool_weights of {a.entries} entries (weights on the host: checks, upload, scan, one stream synchronise, the drain of the "
                         f"env's streams; the first call of a process left out): mean {sum(sets) / len(sets):.1f} us, min {min(sets):.1f}, max {max(sets):.1f} "
                         f"over {len(sets)} calls; first calls " + " ".join("%.0f" % x["set_weights_us"][0] for x in rows[label]))
    if bench:
        lines += ["", f"bench.py --gpus 1 --steps {a.bench_steps} --warmup {a.bench_warmup} (no pool, as always there), the parent's library and this commit's in turn,",
                  "a fresh process per run: env-steps/s, ms per pass, status"]
        lines += [f"{label} {value} {ms} {status}" for label, value, ms, status in bench]
        if a.parent_library:
            lines.append(pc.bench_py_sentence(bench, ".6g"))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
