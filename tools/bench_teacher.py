"""What kickstarting costs.  Off - no teacher configured, the default - against the parent commit's library: bench.py's
env-steps/s and the PPO learner's minibatch-step time (the loop of tools/bench_ppo.py) in alternating pairs, every run a fresh process;
the change passes where its mean lies inside the spread (min..max) of the parent's own runs, or on its better side.  On - reported only:
rollout seconds with teacher labels and the minibatch-step time with teacher_coef > 0 (the second heads pass is the expected cost).

usage: bench_teacher.py --parent-library libcatan_hip.so [--envs N] [--num-steps T] [--ppo-epoch E] [--pairs P] [--on-runs R]
                        [--bench-pairs B] [--out profiles/teacher_bench.txt]

--parent-library: a libcatan_hip.so built from the parent commit, run under this commit's Python (the teacher entry points it lacks are
never called with no teacher configured).  A learner run is two updates of E epochs x 64 minibatches; the second update is reported
(the first captures the policy pass).  minibatch-step ms = minibatches_s / (E x 64)."""
import argparse
import json
import os
import time

import parent_compare as pc


def ppo_child(a):
    pc.use_library(a.library)
    import torch
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    from settlers_of_catan_rl_amd.rollout import RolloutCollector
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy
    from settlers_of_catan_rl_amd.train import PPOTrainer, PPOConfig
    torch.manual_seed(0)
    env = VecCatanEnv(a.envs, seed=0)
    env.random_rollout(0, 600)
    net = CatanPolicy().cuda()
    teach = a.teacher_coef > 0
    col = RolloutCollector(env, net, a.num_steps, seed=0, autocast_dtype=torch.bfloat16, **(dict(teacher=ScriptedPolicy(env)) if teach else {}))
    tr = PPOTrainer(net, PPOConfig(ppo_epoch=a.ppo_epoch, num_mini_batch=64, **(dict(teacher_coef=a.teacher_coef) if teach else {})),
                    autocast_dtype=torch.bfloat16, seed=0)
    out = {"library": a.library or "this commit", "teacher_coef": a.teacher_coef}
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = col.gather_rollouts()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        tr.update(st)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        col.after_rollouts()
        out.update(rollout_s=t1 - t0, update_s=t2 - t1, env_iters=col.iters, minibatch_step_ms=tr.timings["minibatches_s"] / (a.ppo_epoch * 64) * 1e3,
                   values_s=tr.timings["values_s"])
    if tr.teacher is not None:
        out["teacher"] = {k: tr.teacher[k] for k in ("nll", "half_share", "skipped", "rows", "steps")}
    out["invalid_actions"] = env.invalid_action_count()
    out["hbm_gb"] = torch.cuda.max_memory_allocated() / 2 ** 30
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--num-steps", type=int, default=200)
    ap.add_argument("--ppo-epoch", type=int, default=1)
    ap.add_argument("--pairs", type=int, default=2, help="pairs (parent, change) of learner runs with no teacher")
    ap.add_argument("--on-runs", type=int, default=1, help="learner runs with the teacher on (this commit only)")
    ap.add_argument("--on-coef", type=float, default=1.0)
    ap.add_argument("--bench-pairs", type=int, default=2, help="pairs of bench.py runs (0: none)")
    ap.add_argument("--bench-steps", type=int, default=4096)
    ap.add_argument("--bench-warmup", type=int, default=256)
    ap.add_argument("--parent-library")
    ap.add_argument("--out", default=os.path.join(pc.ROOT, "profiles", "teacher_bench.txt"))
    ap.add_argument("--ppo-child", action="store_true")
    ap.add_argument("--bench-child", action="store_true")
    ap.add_argument("--teacher-coef", type=float, default=0.0)
    ap.add_argument("--library")
    a = ap.parse_args()
    if a.ppo_child:
        return ppo_child(a)
    if a.bench_child:
        return pc.bench_py_child(a.library, a.bench_steps, a.bench_warmup)
    sides = ([("parent", a.parent_library)] if a.parent_library else []) + [("change", None)]
    common = ["--envs", str(a.envs), "--num-steps", str(a.num_steps), "--ppo-epoch", str(a.ppo_epoch)]
    ppo, on = [], []

    def learner(label, args):
        res = pc.run_child(__file__, ["--ppo-child"] + args + common, 900, "RESULT ")
        print(label, json.dumps(res), flush=True)
        return res
    bench = pc.bench_py_runs(a.parent_library, a.bench_pairs, a.bench_steps, a.bench_warmup, __file__)
    for r in range(a.pairs):
        for label, lib in pc.order(sides, r, "alternate"):
            ppo.append((label, learner(f"learner run {r} {label}", ["--library", lib] if lib else [])))
    for r in range(a.on_runs):
        on.append(learner(f"learner run {r} teacher on", ["--teacher-coef", str(a.on_coef)]))
    lines = ["Kickstarting from the rule-based player: what it costs off and on (tools/bench_teacher.py)",
             f"commit {pc.commit_of_tree()}; one MI355X, a fresh process per run, the parent's library and this commit's alternating.", ""]
    if bench:
        lines += [f"OFF: bench.py --gpus 1 --steps {a.bench_steps} --warmup {a.bench_warmup}: env-steps/s, ms per pass, status"]
        lines += [f"  {label} {value} {ms} {status}" for label, value, ms, status in bench]
        if a.parent_library:
            lines.append("  " + pc.bench_py_sentence(bench, ".6g"))
        lines.append("")
    if ppo:
        lines += [f"OFF: the PPO learner, {a.envs} games x T = {a.num_steps}, bf16 autocast, {a.ppo_epoch} epoch(s) x 64 minibatches of {a.envs * a.num_steps // 64} rows,",
                  "no teacher configured; the second update of a process: minibatch-step ms, rollout s, value pass s"]
        lines += [f"  {label} {x['minibatch_step_ms']:.3f} {x['rollout_s']:.3f} {x['values_s']:.3f}" for label, x in ppo]
        for key, name in (("minibatch_step_ms", "minibatch-step ms"), ("rollout_s", "rollout s")):
            pv, cv = [x[key] for l, x in ppo if l == "parent"], [x[key] for l, x in ppo if l == "change"]
            if pv and cv:
                lines.append(f"  {name}: " + pc.sentence(cv, pv, False, ".4f"))
        lines.append("")
    if on:
        lines += [f"ON (reported, not bounded): RolloutCollector(teacher=ScriptedPolicy(env)), PPOConfig(teacher_coef={a.on_coef}); the same learner run:",
                  "minibatch-step ms, rollout s, value pass s, HBM GB; the update's read-out"]
        lines += [f"  {x['minibatch_step_ms']:.3f} {x['rollout_s']:.3f} {x['values_s']:.3f} {x['hbm_gb']:.1f}  {json.dumps(x.get('teacher'))}  invalid actions {x['invalid_actions']}" for x in on]
        off = [x for l, x in ppo if l == "change"]
        if off:
            m = lambda xs, k: sum(x[k] for x in xs) / len(xs)
            lines.append(f"  against this commit's runs without a teacher: minibatch step {m(on, 'minibatch_step_ms'):.3f} ms vs {m(off, 'minibatch_step_ms'):.3f} ms, "
                         f"rollout {m(on, 'rollout_s'):.3f} s vs {m(off, 'rollout_s'):.3f} s ({on[0]['env_iters']} env iterations, three more launches each: the player, the completion, the store)")
        lines.append("")
    lines += ["NOT timed: the three kernels on their own (hipEvents around catan_complete_action_rows / catan_collector_label / catan_imitation_loss),",
              "more than one rank, the LSTM path (not supported), teacher_only, the league rollout with a teacher, any effect on learning."]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
