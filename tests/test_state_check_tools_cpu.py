"""The host side of the state check without a device: tools/check_states.py and tools/make_start_pool.py --check over the
numpy restatement of the rules, the message that names the bad blobs, and the option's way through run_evaluation_episodes."""
import os
import sys

import numpy as np
import pytest
import torch

import state_check_cases as cases
import state_check_reference as ref
from settlers_of_catan_rl_amd import evaluation, position, start_pool

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_check_states_reports_per_entry_and_by_exit_status(oracle, tmp_path, capsys):
    import check_states
    legal = cases.legal_pool()
    live = legal[spec_field(legal, "winner") == 0][:40]
    good, bad, none = str(tmp_path / "pool.npz"), str(tmp_path / "rec.npz"), str(tmp_path / "none.npz")
    start_pool.save(start_pool.StartPool(live), good)
    name, blob, rules = cases.planted()[12]
    np.savez(bad, start_blob=legal[3], final_blob=blob, actions=np.zeros((5, 18), dtype=np.int32))
    np.savez(none, actions=np.zeros((5, 18), dtype=np.int32))
    assert check_states.main([good], check=ref.state_check) == 0
    assert "40 entries, 0 break a rule" in capsys.readouterr().out
    assert check_states.main([good, bad], check=ref.state_check) == 1
    out = capsys.readouterr().out
    assert f"{bad}:final_blob: 1 entries, 1 break a rule" in out and "entry 0: " + ", ".join(sorted(rules, key=ref.RULES.index)) in out
    assert f"{bad}:start_blob: 1 entries, 0 break a rule" in out
    assert check_states.main([none], check=ref.state_check) == 2


def spec_field(blobs, name):
    from settlers_of_catan_rl_amd import spec
    return spec.state_field(blobs, name)[:, 0]


def test_make_start_pool_check_refuses_to_write(oracle, tmp_path, capsys, monkeypatch):
    import make_start_pool
    legal = cases.legal_pool()
    live = legal[spec_field(legal, "winner") == 0][:16].copy()
    monkeypatch.setattr(start_pool.StartPool, "from_records", classmethod(lambda cls, records, **kw: start_pool.StartPool(live)))
    out = str(tmp_path / "pool.npz")
    assert make_start_pool.main(["-o", out, "--check", "unused.npz"], check=ref.state_check) == 0 and os.path.exists(out)
    os.remove(out)
    live[5] = cases.planted()[13][1]
    assert make_start_pool.main(["-o", out, "--check", "unused.npz"], check=ref.state_check) == 1 and not os.path.exists(out)
    said = capsys.readouterr().out
    assert "not written" in said and "blob 5: card_conservation" in said
    assert make_start_pool.main(["-o", out, "unused.npz"]) == 0 and os.path.exists(out)          # without --check nothing is asked


def test_describe_bad_names_the_first_eight():
    v = np.zeros(20, dtype=np.uint64)
    v[[2, 3, 5, 7, 8, 9, 11, 13, 17, 19]] = 1 << 9
    v[3] |= 1 << 0
    text = position.describe_bad(v)
    assert text.startswith("10 of 20 blobs break the state rules: blob 2: resource_conservation; blob 3: range_board, resource_conservation; ")
    assert "blob 13" in text and "blob 17" not in text and text.endswith("(and 2 more)")
    assert position.describe_bad(torch.from_numpy(v.view(np.int64))) == text


class _Refusing(object):
    """an env that takes note of the import and ends the run there"""
    n, device = 4, torch.device("cpu")

    def __init__(self):
        self.calls = []

    def import_state(self, blobs, **kw):
        self.calls.append((tuple(blobs.shape), kw))
        raise KeyboardInterrupt


@pytest.mark.parametrize("check", [False, True])
def test_run_evaluation_episodes_passes_the_option_through(oracle, check):
    env = _Refusing()
    with pytest.raises(KeyboardInterrupt):
        evaluation.run_evaluation_episodes(env, [None] * 4, np.tile(np.arange(1, 5), (4, 1)), start_blobs=cases.legal_pool()[:3], check_blobs=check)
    assert env.calls == [((4, 736), {"check": True} if check else {})]
