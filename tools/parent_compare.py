"""The acceptance rule behind "costs nothing when off" (DESIGN.md 6), stated once, and the plumbing the tools/bench_<feature>.py share.

The rule: the change and the parent commit's library (run under this commit's Python: _lib.use_library) are measured in fresh
processes, one per run, in an order that alternates or rotates from round to round so that drift of the machine hits both alike.  The
change passes where the MEAN of its runs lies inside the spread min..max of the parent's own runs, bounds included, or on its better
side (`verdict`; which side is better is the caller's to say: higher for env-steps/s, lower for a time).

No import of torch or of the package at module level: a tool's parent process must not touch the device before its children have run,
and --help needs neither."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)                # the package, for the tools that import this module first


def verdict(change, parent, higher_is_better):
    """-> (mean of `change`, where it lies against min..max of `parent`): "inside" (bounds included), or "ABOVE" / "BELOW" followed by
    " (better than)" / " (WORSE than)" """
    if not change or not parent:
        raise ValueError("verdict needs at least one run of the change and one of the parent")
    mean = sum(change) / len(change)
    if min(parent) <= mean <= max(parent):
        return mean, "inside"
    above = mean > max(parent)
    return mean, ("ABOVE" if above else "BELOW") + (" (better than)" if above == bool(higher_is_better) else " (WORSE than)")


def sentence(change, parent, higher_is_better, fmt=".2f"):
    """the one wording of a verdict"""
    mean, where = verdict(change, parent, higher_is_better)
    return f"the change's mean {mean:{fmt}} lies {where} the parent's spread {min(parent):{fmt}}..{max(parent):{fmt}}"


def order(configs, r, how):
    """-> the configurations in the order of round r.  "alternate": as given in even rounds, reversed in odd ones (parent, change, change,
    parent, ...); "rotate": starting at r % len(configs), so that none always runs behind the same neighbour; "fixed": as given"""
    configs = list(configs)
    if how == "alternate":
        return configs if r % 2 == 0 else configs[::-1]
    if how == "rotate":
        return configs[r % len(configs):] + configs[:r % len(configs)]
    if how == "fixed":
        return configs
    raise ValueError(f"order: how = {how!r}")


def run_child(script, args, timeout, prefix):
    """Runs `script args` in a fresh process -> its last output line that starts with `prefix`, parsed as JSON from its first brace on.
    A non-zero exit or no such line prints the child's output and ends the caller: nothing is retried, nothing more is started on the
    device."""
    p = subprocess.run([sys.executable, os.path.abspath(script)] + list(args), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    text = p.stdout.decode("utf-8", "replace")
    res = [ln for ln in text.splitlines() if ln.startswith(prefix) and "{" in ln]
    if p.returncode != 0 or not res:
        print(text)
        raise SystemExit(f"{os.path.basename(script)} {' '.join(args)} failed with exit code {p.returncode}"
                         + ("" if res else f" (no line starting with {prefix!r})"))
    return json.loads(res[-1][res[-1].index("{"):])


def use_library(library):
    """a child's first step: `library` (a parent commit's libcatan_hip.so; None: this commit's own) under this commit's Python"""
    if library:
        from settlers_of_catan_rl_amd import _lib
        _lib.use_library(library)


def bench_py_child(library, steps, warmup):
    """bench.py as it stands, in this process, under `library`"""
    import runpy
    use_library(library)
    sys.argv = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
    runpy.run_path(sys.argv[0], run_name="__main__")


def bench_py_runs(parent_library, pairs, steps, warmup, script, how="alternate", timeout=600):
    """`pairs` rounds of bench.py under the parent's library (where one is given) and this commit's, a fresh process each: `script
    --bench-child` must end in bench_py_child.  -> rows (label, value, ms_per_step, status), label "parent" or "change", in run order"""
    sides, rows = ([("parent", parent_library)] if parent_library else []) + [("change", None)], []
    for r in range(pairs):
        for label, lib in order(sides, r, how):
            j = run_child(script, ["--bench-child", "--bench-steps", str(steps), "--bench-warmup", str(warmup)] + (["--library", lib] if lib else []), timeout, "{")
            rows.append((label, j.get("value"), j.get("ms_per_step"), j.get("status")))
            print("bench.py run {} {} {} {} {}".format(r, *rows[-1]), flush=True)
    return rows


def bench_py_sentence(rows, fmt):
    """-> the verdict on bench_py_runs' rows (env-steps/s: higher is better), None where one side did not run"""
    parent, change = [v for l, v, _, _ in rows if l == "parent"], [v for l, v, _, _ in rows if l == "change"]
    return sentence(change, parent, True, fmt) if parent and change else None


def bench_py_section(a, out, unused, script):
    """bench_py_runs with a.parent_library, a.bench_pairs, a.bench_steps and a.bench_warmup, its rows and verdict written to the open
    file `out`: the section of a feature tool that shows bench.py is where the parent's is with the feature (`unused`) not in use"""
    rows = bench_py_runs(a.parent_library, a.bench_pairs, a.bench_steps, a.bench_warmup, script)
    parent = [v for l, v, _, _ in rows if l == "parent"]
    text = ("\nbench.py --gpus 1 --steps {} --warmup {} with the {} unused, a fresh process per run, the parent's library and this\n"
            "commit's alternating: env-steps/s, ms per pass, status\n".format(a.bench_steps, a.bench_warmup, unused)
            + "".join("  {} {} {} {}\n".format(*row) for row in rows)
            + "  {} (parent's mean {:.5e})\n".format(bench_py_sentence(rows, ".5e"), sum(parent) / len(parent)))
    print(text, flush=True)
    out.write(text)
    out.flush()


def commit_of_tree():
    """`git rev-parse HEAD` of the tree this file lies in (+ a mark when the tree has uncommitted changes)"""
    try:
        head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout.decode().strip()
        dirty = subprocess.run(["git", "status", "--porcelain"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout.strip()
        return head + (" + uncommitted changes" if dirty else "")
    except (OSError, subprocess.CalledProcessError):
        return "unknown (no git metadata beside this tree)"


def step_call_times(env, calls, warmup, between=None):
    """-> {"catan_step_us", "catan_step_deferred_us"}: microseconds per call, host clock around `calls` calls behind `warmup` calls.  A
    call is the uniform-random sampler, then env.step or env.step_deferred(window=4); a loop ends in the flush (deferred) and a device
    synchronise.  between(name, "warmed") runs before the timed calls of a loop and between(name, "timed") after them: where a tool
    resets and reads its own counters."""
    import torch
    out, step_idx = {}, 0
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
        run(warmup)
        if between:
            between(name, "warmed")
        t0 = time.perf_counter()
        run(calls)
        out[name + "_us"] = (time.perf_counter() - t0) / calls * 1e6
        if between:
            between(name, "timed")
    return out


def event_call_times(calls, reps, rounds, warm=10):
    """calls: {name: function}.  After `warm` calls of each, `rounds` rounds that alternate between them, hipEvents around `reps`
    back-to-back calls.  -> {name: {"device_us": [min, median, max], "host_issue_us": [min, median, max]}} per call: the time between the
    events, and the host's time to issue the calls without waiting for the device (a device figure close to it is launch-bound and only
    bounds the kernel from above)."""
    import torch
    for fn in calls.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    us, host = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            host[k].append((time.perf_counter() - t0) * 1e6 / reps)
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    mmm = lambda xs: [min(xs), sorted(xs)[len(xs) // 2], max(xs)]
    return {k: {"device_us": mmm(us[k]), "host_issue_us": mmm(host[k])} for k in calls}


def UniformRandom():
    """the uniform-random sampler as a seat of evaluation games: scripted.RandomPolicy, unbound (imported at the call: see the top)"""
    from settlers_of_catan_rl_amd.scripted import RandomPolicy
    return RandomPolicy()
