"""What the state check costs, measured.

  off      bench.py with the parent commit's library and this commit's in alternating fresh-process pairs: the check is never called
           there, and the change passes by parent_compare.verdict
  kernel   catan_state_check per call at 4 096 and 65 536 blobs, hipEvents around back-to-back calls: microseconds, and the 2 944 bytes a
           blob is read with as bytes per second against the 8 TB/s HBM peak (MI355X_MICROARCH.md).  The same blobs every call: 4 096
           blobs are 12 MB and stay in the caches, 65 536 are 193 MB
  options  import_state and set_start_pool of 4 096 blobs with and without check=True: host clock around the call and a device
           synchronise, alternating

usage: bench_state_check.py [--parent-library libcatan_hip.so] [--bench-pairs B] [--reps R] [--rounds N] [--out profiles/state_check_bench.txt]"""
import argparse
import json
import os
import time

import parent_compare as pc

BLOB_BYTES = 2944
HBM_PEAK = 8.0e12


def _legal_blobs(n):
    """n legal blobs: live games of a random rollout"""
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    env = VecCatanEnv(n, seed=4, auto_reset=False)
    env.random_rollout(0, 60)
    return env.export_state()


def kernel_child(a):
    import torch
    from settlers_of_catan_rl_amd import position
    out = {}
    for cnt in (4096, 65536):
        bt = _legal_blobs(cnt).t().contiguous()
        viol, n_bad = position.check_transposed(bt, want_count=True)
        assert n_bad == 0 and not viol.view(torch.int64).any()
        # the entry point itself on buffers of the caller's: nothing but the kernel is launched between the events
        from settlers_of_catan_rl_amd import _lib
        from settlers_of_catan_rl_amd.env import _ptr, _stream
        L, out_words, stream = _lib.lib(), torch.zeros(cnt, dtype=torch.int64, device=bt.device), _stream()
        t = pc.event_call_times({"check": lambda: _lib.check(L.catan_state_check(_ptr(bt), cnt, _ptr(out_words), None, stream))}, a.reps, a.rounds)["check"]
        assert not out_words.any()
        out[str(cnt)] = t
    print("RESULT " + json.dumps(out), flush=True)


def options_child(a):
    import torch
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    n = 4096
    blobs = _legal_blobs(n)
    env = VecCatanEnv(n, seed=5)
    calls = {"import_state": lambda c: env.import_state(blobs, check=c), "set_start_pool": lambda c: env.set_start_pool(blobs, check=c)}
    rows = {f"{k} check={c}": [] for k in calls for c in (False, True)}
    for r in range(a.rounds + 2):
        for k, fn in calls.items():
            for c in pc.order([False, True], r, "alternate"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(c)
                torch.cuda.synchronize()
                if r >= 2:                                   # two rounds to warm up
                    rows[f"{k} check={c}"].append((time.perf_counter() - t0) * 1e6)
    print("RESULT " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-library")
    ap.add_argument("--bench-pairs", type=int, default=5, help="pairs of bench.py runs (0: none)")
    ap.add_argument("--bench-steps", type=int, default=4096)
    ap.add_argument("--bench-warmup", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(pc.ROOT, "profiles", "state_check_bench.txt"))
    ap.add_argument("--child", choices=["kernel", "options"])
    ap.add_argument("--bench-child", action="store_true")
    ap.add_argument("--library")
    a = ap.parse_args()
    if a.bench_child:
        return pc.bench_py_child(a.library, a.bench_steps, a.bench_warmup)
    if a.child:
        return {"kernel": kernel_child, "options": options_child}[a.child](a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        out.write(f"The state check (DESIGN.md 8.17), measured by tools/bench_state_check.py on one MI355X; commit {pc.commit_of_tree()}\n")
        if a.bench_pairs and a.parent_library:
            pc.bench_py_section(a, out, "state check", __file__)
        common = ["--reps", str(a.reps), "--rounds", str(a.rounds)]
        res = pc.run_child(__file__, ["--child", "kernel"] + common, 600, "RESULT ")
        lines = ["", f"catan_state_check per call, hipEvents around {a.reps} back-to-back calls, {a.rounds} rounds: min / median / max microseconds; bytes read",
                 f"({BLOB_BYTES} per blob) per second at the median against the 8 TB/s HBM peak; the host's time to issue a call beside it (a device figure",
                 "close to it is launch-bound and only bounds the kernel from above)"]
        for cnt, t in res.items():
            d, h = t["device_us"], t["host_issue_us"]
            rate = int(cnt) * BLOB_BYTES / (d[1] * 1e-6)
            lines.append(f"  {int(cnt):6d} blobs  device {d[0]:8.2f} {d[1]:8.2f} {d[2]:8.2f}   host issue {h[0]:7.2f} {h[1]:7.2f} {h[2]:7.2f}   "
                         f"{rate / 1e12:6.3f} TB/s = {rate / HBM_PEAK * 100:5.1f} % of the peak")
        text = "\n".join(lines) + "\n"
        print(text, flush=True)
        out.write(text)
        out.flush()
        res = pc.run_child(__file__, ["--child", "options"] + common, 600, "RESULT ")
        lines = ["", f"import_state and set_start_pool of 4 096 blobs on a 4 096-game env, microseconds per call (host clock, device synchronised), {a.rounds} calls each,",
                 "check=False and check=True alternating; check=True adds the kernel, one 8-byte read and its wait"]
        for k, v in res.items():
            lines.append(f"  {k:28s} min {min(v):9.1f}   median {sorted(v)[len(v) // 2]:9.1f}   max {max(v):9.1f}")
        text = "\n".join(lines) + "\n"
        print(text, flush=True)
        out.write(text)


if __name__ == "__main__":
    main()
