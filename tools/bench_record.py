"""What the game recorder costs a step: catan_step and catan_step_deferred in microseconds per call at 65 536 games with
recording off, with 64 and with 4 096 slots recording (armed NOW: every call appends a row per slot), three runs each, every run a
fresh process; the configurations alternate inside a round and their order rotates from round to round, so that drift of the machine
hits them alike.

usage: bench_record.py [--games N] [--calls K] [--warmup W] [--runs R] [--parent-library libcatan_hip.so] [--off-only] [--out profiles/record_bench.txt]

--parent-library: a libcatan_hip.so built from the parent commit; its off-path (the only one it has) runs as a fourth configuration in
every round.  The off case of this commit passes if its mean lies inside the spread (min..max) of the parent's runs (or below it).
A call is: the uniform-random sampler (catan_sample_random_actions), then the step - the same in every configuration.  Timed with the
host clock around K calls that end in a device synchronise."""
import argparse
import json
import os

import parent_compare as pc


def child(a):
    pc.use_library(a.library)                       # the parent commit's library under this commit's Python (the off-path uses nothing new)
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    env = VecCatanEnv(a.games, seed=1)
    if a.slots:
        stride = a.games // a.slots
        env.enable_recording(list(range(0, a.slots * stride, stride)), capacity=8192)
        env.arm_recording()
    out = {"slots": a.slots, "library": a.library or "this commit"}
    out.update(pc.step_call_times(env, a.calls, a.warmup))
    if a.slots:
        st = env.recording_status()
        out["appended_rows_per_slot"] = float(st[:, 2].float().mean())
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-library")
    ap.add_argument("--out", default=os.path.join(pc.ROOT, "profiles", "record_bench.txt"))
    ap.add_argument("--off-only", action="store_true", help="only the configurations without slots (the comparison with the parent)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--slots", type=int, default=0)
    ap.add_argument("--library")
    a = ap.parse_args()
    if a.child:
        return child(a)
    configs = [("off", 0, None), ("64 slots", 64, None), ("4096 slots", 4096, None)]
    if a.parent_library:
        configs.insert(0, ("parent, off", 0, a.parent_library))
    rows = {c[0]: [] for c in configs}
    if a.off_only:
        configs = [c for c in configs if c[1] == 0]
    for r in range(a.runs):
        for label, slots, lib in pc.order(configs, r, "rotate"):  # (no configuration always runs behind the same neighbour)
            res = pc.run_child(__file__, ["--child", "--games", str(a.games), "--calls", str(a.calls), "--warmup", str(a.warmup), "--slots", str(slots)]
                               + (["--library", lib] if lib else []), 300, "RESULT ")
            rows[label].append(res)
            print(f"run {r} {label:12s} {json.dumps(res)}", flush=True)
    lines = ["Game recorder: what recording costs a step (tools/bench_record.py)",
             f"commit {pc.commit_of_tree()}; {a.games} games, {a.calls} timed calls behind {a.warmup} warm-up calls, {a.runs} runs each,",
             "a fresh process per run, configurations alternating; a call = catan_sample_random_actions + the step; host clock around the calls,",
             "ending in a device synchronise.  Microseconds per call.", ""]
    for key in ("catan_step_us", "catan_step_deferred_us"):
        lines.append(key[:-3])
        for label, _, _ in configs:
            v = [x[key] for x in rows[label]]
            lines.append(f"  {label:12s} runs {' '.join(f'{x:8.2f}' for x in v)}   mean {sum(v) / len(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}")
        if a.parent_library:
            lines.append("  off against the parent: " + pc.sentence([x[key] for x in rows["off"]], [x[key] for x in rows["parent, off"]], False))
        lines.append("")
    for label, slots, _ in configs:
        if slots:
            lines.append(f"{label}: {rows[label][0]['appended_rows_per_slot']:.0f} rows appended per slot in a run (both loops and their warm-ups)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
