"""Generates tests/golden/act_stats.npz from the imported upstream reference (development container only): what the
reference's OWN net (`build_agent_model()` with the fixture weights of tests/policy_fixture.py, salt "ff:") returns from
`act(deterministic=True, return_entropy=True, log_specific_action_output=True)` as SINGLE-ROW calls - the way its offline
evaluator calls it (evaluation/evaluation_manager.py:69-78) - on the real oracle observations of tests/golden/policy_small.npz
(its "ff_" inputs; they are not stored again).

  free_*      every row, type head free: entropy, log tuples, arg-max actions, joint log-prob
  forced_*    rows with the type forced (condition_on_action_type), every legal type represented (up to 4 rows per type)

The log tuples (action_type or None, head, prob, n_available, action) are stored as the record of
policy._ActionHeads.forward(stats=True): [type prob, legal types, specific head prob, its legal columns] plus the specific
head's id (-1: none) and action.  The data is inputs and outputs only; no reference source is stored.

usage: python tools/gen_golden_eval_stats.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness  # noqa: E402,F401  (puts the reference on sys.path)
from gen_golden import _ref_policy_inputs, _flat_actions  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def _record(log, forced):
    """the reference's tuple list -> [type prob, legal types, specific prob, specific legal columns], specific head, its action"""
    rec, head, act = [1.0, 0.0, 0.0, 0.0], -1, -1
    for t, h, p, n, a in log:
        if t is None:
            assert h == 0 and not forced
            rec[0], rec[1] = float(p), float(n)
        else:
            rec[2], rec[3], head, act = float(p), float(n), int(h), int(a)
    return rec, head, act


def gen_act_stats(per_type=4):
    import torch
    import policy_fixture as pf
    import RL.models.build_agent_model as bam
    g = np.load(os.path.join(OUT, "policy_small.npz"))
    x, B = pf.decode_inputs(g, "ff_")
    torch.manual_seed(0)
    ref = bam.build_agent_model()
    sd = ref.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items() if v.numel() > 0 and not k.startswith("value_normaliser.")}
    full = dict(sd); full.update(pf.fixture_state_dict(shapes, "ff:"))
    ref.load_state_dict(full, strict=True)
    ref.eval()
    names = sorted(shapes)
    assert [pf.tensor_crc(full[k]) for k in names] == [int(c) for c in g["ff_param_crc"]]
    obs, masks = _ref_policy_inputs(x)
    # the reference's act WRITES into its own log-prob mask tables on a one-row call (a squeezed 0-d index returns a view, and
    # `head_prob_mask[action_type_mask, ...] = 1.0` stores through it when the type is not PlayDevelopmentCard): restore them
    # before every call, so that each record is what the net computes, independent of the order of the calls
    tables = [t for m in ref.action_head_module.log_prob_masks if m is not None for t in m.values()]
    pristine = [t.clone() for t in tables]

    def one(i, forced=None):
        for t, p in zip(tables, pristine):
            t.copy_(p)
        o = {k: v[i:i + 1].clone() for k, v in obs.items()}
        m = [mk[:, i:i + 1].clone() if hi in (1, 6, 9) else mk[i:i + 1].clone() for hi, mk in enumerate(masks)]
        with torch.no_grad():
            v, a, lp, _, ent, log = ref.act(o, None, None, m, deterministic=True, return_entropy=True, condition_on_action_type=forced,
                                            log_specific_action_output=True)
        rec, head, act = _record(log, forced is not None)
        return float(ent), rec, head, act, _flat_actions(a, 1).numpy()[0], float(lp.reshape(-1)[0])

    out = {}

    def store(prefix, rows, forced):
        res = [one(i, None if f < 0 else int(f)) for i, f in zip(rows, forced)]
        out[prefix + "rows"] = np.asarray(rows, dtype=np.int16)
        out[prefix + "entropy"] = np.array([r[0] for r in res], dtype=np.float32)
        out[prefix + "log"] = np.array([r[1] for r in res], dtype=np.float32)
        out[prefix + "log_head"] = np.array([r[2] for r in res], dtype=np.int8)
        out[prefix + "log_action"] = np.array([r[3] for r in res], dtype=np.int8)
        out[prefix + "actions"] = np.stack([r[4] for r in res]).astype(np.int8)
        out[prefix + "logp"] = np.array([r[5] for r in res], dtype=np.float32)

    store("free_", list(range(B)), [-1] * B)
    legal = x["masks"][:, :13].numpy() > 0
    rows, types = [], []
    for t in range(13):
        for i in np.flatnonzero(legal[:, t])[:per_type]:
            rows.append(int(i)); types.append(t)
    store("forced_", rows, types)
    out["forced_type"] = np.asarray(types, dtype=np.int8)
    path = os.path.join(OUT, "act_stats.npz")
    np.savez_compressed(path, **out)
    return {"rows": B, "forced_rows": len(rows), "forced_types": sorted(set(types)), "bytes": os.path.getsize(path)}


if __name__ == "__main__":
    print("act_stats", gen_act_stats())
