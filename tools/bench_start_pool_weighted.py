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
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _use_library(path):
    """the parent commit's library under this commit's Python"""
    os.environ["CATAN_ALLOW_STALE_LIB"] = "1"
    from settlers_of_catan_rl_amd import _lib
    _lib.LIB_PATH = os.path.abspath(path)


def child(a):
    if a.library:
        _use_library(a.library)
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
    step_idx = 0
    for name in ("catan_step", "catan_step_deferred"):
        deferred = name == "catan_step_deferred"

        def run(k):
            nonlocal step_idx
            for _ in range(k):
                acts = env.sample_random_actions(step_idx)
                step_idx += 1
                if deferred:
                    env.step_deferred(acts, window=4)
                else:
                    env.step(acts)
            if deferred:
                env.step_flush()
            torch.cuda.synchronize()
        run(a.warmup)
        if a.mode != "off":
            env.start_pool_counts(reset=True)
        t0 = time.perf_counter()
        run(a.calls)
        out[name + "_us"] = (time.perf_counter() - t0) / a.calls * 1e6
        if a.mode != "off":
            c = env.start_pool_counts(reset=True)
            out[name + "_deals"] = [c["pool"], c["fresh"]]
            out[name + "_entries_hit"] = int((c["per_entry"] > 0).sum())
        if a.mode == "weighted+outcomes":
            o = env.start_pool_outcomes(reset=True)
            out[name + "_tallied"] = [o["seen"], o["skipped"]]
    print("RESULT " + json.dumps(out), flush=True)


def bench_child(a):
    """bench.py as it stands, in this process, under the given library"""
    import runpy
    if a.library:
        _use_library(a.library)
    sys.argv = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup)]
    runpy.run_path(sys.argv[0], run_name="__main__")


def _spawn(args, timeout):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    return p.returncode, p.stdout.decode("utf-8", "replace")


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "start_pool_weighted_bench.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--bench-child", action="store_true")
    ap.add_argument("--mode", default="off", choices=["off", "uniform", "weighted", "weighted+outcomes"])
    ap.add_argument("--library")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.bench_child:
        return bench_child(a)
    configs = [("off", "off", None), (f"uniform, {a.entries} entries", "uniform", None), (f"weighted, {a.entries} entries", "weighted", None),
               ("weighted + outcomes", "weighted+outcomes", None)]
    if a.parent_library:
        configs = [c for label, mode, _ in configs for c in ((f"parent, {label}", mode, a.parent_library), (label, mode, None))]
    rows = {c[0]: [] for c in configs}
    for r in range(a.runs):
        # (the order rotates from round to round: no configuration always runs behind the same neighbour)
        for label, mode, lib in configs[r % len(configs):] + configs[:r % len(configs)]:
            rc, text = _spawn(["--child", "--games", str(a.games), "--calls", str(a.calls), "--warmup", str(a.warmup), "--entries", str(a.entries),
                               "--mode", mode] + (["--library", lib] if lib else []), 300)
            res = [ln for ln in text.splitlines() if ln.startswith("RESULT ")]
            if rc != 0 or not res:
                print(text)
                raise SystemExit(f"run {r} of {label!r} failed with exit code {rc}")      # nothing more is started on the device
            rows[label].append(json.loads(res[-1][7:]))
            print(f"run {r} {label:34s} {res[-1][7:]}", flush=True)
    bench = []
    for r in range(a.bench_runs):
        for label, lib in ([("parent", a.parent_library)] if a.parent_library else []) + [("change", None)]:
            rc, text = _spawn(["--bench-child", "--bench-steps", str(a.bench_steps), "--bench-warmup", str(a.bench_warmup)] + (["--library", lib] if lib else []), 900)
            res = [ln for ln in text.splitlines() if ln.startswith("{") and '"value"' in ln]
            if rc != 0 or not res:
                print(text)
                raise SystemExit(f"bench.py run {r} ({label}) failed with exit code {rc}")
            j = json.loads(res[-1])
            bench.append((label, j.get("value"), j.get("ms_per_step"), j.get("status")))
            print(f"bench.py run {r} {label} {j.get('value')} {j.get('ms_per_step')} {j.get('status')}", flush=True)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode().strip()
    except OSError:
        commit = ""
    lines = ["Start pool, weighted picks and outcome tallies: what they cost a step (tools/bench_start_pool_weighted.py)",
             f"commit {commit or 'unknown (no git checkout where it ran)'}; {a.games} games, {a.calls} timed calls behind {a.warmup} warm-up calls, {a.runs} runs each,",
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
            pv, ov = [x[key] for x in rows["parent, " + label]], [x[key] for x in rows[label]]
            mean = sum(ov) / len(ov)
            where = "inside" if min(pv) <= mean <= max(pv) else ("BELOW (faster than)" if mean < min(pv) else "ABOVE (slower than)")
            lines.append(f"  {label} against the parent: mean {mean:.2f} {where} the parent's spread {min(pv):.2f}..{max(pv):.2f}")
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
        pv, cv = [b[1] for b in bench if b[0] == "parent"], [b[1] for b in bench if b[0] == "change"]
        if pv and cv:
            mean = sum(cv) / len(cv)
            where = "inside" if min(pv) <= mean <= max(pv) else ("ABOVE (faster than)" if mean > max(pv) else "BELOW (slower than)")
            lines.append(f"the change's mean {mean:.6g} lies {where} the parent's spread {min(pv):.6g}..{max(pv):.6g}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
