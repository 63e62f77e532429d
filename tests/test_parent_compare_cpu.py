"""tools/parent_compare.py - the acceptance rule of "costs nothing when off" (the change's mean against the inclusive min..max of the
parent's runs), the run orders, the fresh-process plumbing - and _lib.use_library, which runs this Python over another commit's
library; the seven tools built on them start without torch and no longer reach into _lib's private state.  No GPU needed."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from settlers_of_catan_rl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)
import parent_compare as pc  # noqa: E402

SEVEN = ["bench_record", "bench_start_pool", "bench_start_pool_weighted", "bench_teacher", "bench_trader", "bench_playout", "bench_scripted"]


def test_verdict_bounds_are_inclusive():
    assert pc.verdict([10.0], [10.0, 12.0], False) == (10.0, "inside")
    assert pc.verdict([12.0], [12.0, 10.0, 11.0], True) == (12.0, "inside")
    assert pc.verdict([9.0, 11.0], [10.0, 12.0], True) == (10.0, "inside")           # the MEAN of the change's runs, not each of them


@pytest.mark.parametrize("value, higher_is_better, where", [
    (9.999, False, "BELOW (better than)"), (9.999, True, "BELOW (WORSE than)"),
    (12.001, False, "ABOVE (WORSE than)"), (12.001, True, "ABOVE (better than)")])
def test_verdict_outside_names_the_side_and_whether_it_is_the_better_one(value, higher_is_better, where):
    assert pc.verdict([value], [10.0, 12.0], higher_is_better) == (value, where)
    assert pc.sentence([value], [10.0, 12.0], higher_is_better, ".3f") == f"the change's mean {value:.3f} lies {where} the parent's spread 10.000..12.000"


def test_verdict_single_parent_run_and_empty_lists():
    assert pc.verdict([5.0], [5.0], True)[1] == "inside"
    assert pc.verdict([5.5], [5.0], True)[1] == "ABOVE (better than)" and pc.verdict([4.5], [5.0], True)[1] == "BELOW (WORSE than)"
    assert pc.sentence([5.0], [5.0], False) == "the change's mean 5.00 lies inside the parent's spread 5.00..5.00"
    for change, parent in (([1.0], []), ([], [1.0])):
        with pytest.raises(ValueError):
            pc.verdict(change, parent, True)


def test_order_is_the_two_schedules_of_the_tools():
    sides = ["parent", "change"]
    assert [pc.order(sides, r, "alternate") for r in range(3)] == [["parent", "change"], ["change", "parent"], ["parent", "change"]]
    c = ["p", "a", "b", "c"]
    assert [pc.order(c, r, "rotate") for r in range(5)] == [["p", "a", "b", "c"], ["a", "b", "c", "p"], ["b", "c", "p", "a"], ["c", "p", "a", "b"],
                                                            ["p", "a", "b", "c"]]
    assert pc.order(tuple(sides), 1, "fixed") == sides and sides == ["parent", "change"]
    with pytest.raises(ValueError):
        pc.order(sides, 0, "shuffle")


def _script(tmp_path, name, body):
    p = tmp_path / name
    p.write_text(body)
    return str(p)


def test_run_child_returns_the_last_matching_line_parsed(tmp_path):
    s = _script(tmp_path, "two.py", 'import sys\nprint("RESULT {\\"x\\": 1}")\nprint("noise")\nprint("RESULT " + \'{"x": 2, "arg": "%s"}\' % sys.argv[1])\nprint("{}")\n')
    assert pc.run_child(s, ["seven"], 60, "RESULT ") == {"x": 2, "arg": "seven"}
    s = _script(tmp_path, "bench_like.py", 'print(\'{"value": null, "status": "started"}\')\nprint("text")\nprint(\'{"metric": "m", "value": 3.5, "status": "ok"}\')\n')
    assert pc.run_child(s, [], 60, "{") == {"metric": "m", "value": 3.5, "status": "ok"}


def test_run_child_failures_end_the_caller_and_nothing_more_is_started(tmp_path, capsys):
    failing = _script(tmp_path, "exit3.py", 'import sys\nprint("RESULT {\\"x\\": 1}")\nprint("the reason")\nsys.exit(3)\n')
    with pytest.raises(SystemExit) as e:
        pc.run_child(failing, [], 60, "RESULT ")
    assert "exit code 3" in str(e.value.code) and "the reason" in capsys.readouterr().out          # the child's output is shown
    silent = _script(tmp_path, "silent.py", 'print("result {}")\nprint("RESULT without a brace")\n')
    with pytest.raises(SystemExit) as e:
        pc.run_child(silent, [], 60, "RESULT ")
    assert "exit code 0" in str(e.value.code)
    marker = tmp_path / "started"
    second = _script(tmp_path, "second.py", 'open(%r, "w").close()\nprint("RESULT {}")\n' % str(marker))
    with pytest.raises(SystemExit):
        for s in (failing, second):                   # a tool's loop over its children
            pc.run_child(s, [], 60, "RESULT ")
    assert not marker.exists()
    assert pc.run_child(second, [], 60, "RESULT ") == {} and marker.exists()


def test_bench_py_sentence_reads_the_rows():
    rows = [("parent", 10.0, 1.0, "ok"), ("change", 12.5, 0.9, "ok"), ("change", 13.5, 0.9, "ok"), ("parent", 12.0, 1.0, "ok")]
    assert pc.bench_py_sentence(rows, ".1f") == "the change's mean 13.0 lies ABOVE (better than) the parent's spread 10.0..12.0"
    assert pc.bench_py_sentence(rows[1:3], ".1f") is None


def test_use_library_binds_what_the_library_exports_and_accepts_its_hash(monkeypatch):
    import cpu_abi_driver as drv
    L = drv.cpu_lib()
    exported = [n for n in _lib.declared_symbols() if hasattr(L, n)]
    assert 20 <= len(exported) < len(_lib.declared_symbols())
    missing = next(n for n in _lib.declared_symbols() if n not in exported and n not in _lib._OPTIONAL)
    assert sorted(_lib.bind(C.CDLL(drv.CPU_LIB), missing_ok=True)) == exported
    with pytest.raises(AttributeError):
        _lib.bind(C.CDLL(drv.CPU_LIB))                # the default: a required entry point it lacks raises
    with pytest.raises(AttributeError):
        _lib.bind(C.CDLL(drv.CPU_LIB), [missing])
    for name in ("_lib", "_foreign", "LIB_PATH"):     # (put back when the test ends)
        monkeypatch.setattr(_lib, name, getattr(_lib, name))
    monkeypatch.delenv("CATAN_ALLOW_STALE_LIB", raising=False)
    _lib._lib = None
    _lib.use_library(os.path.relpath(drv.CPU_LIB))
    assert _lib.LIB_PATH == drv.CPU_LIB
    loaded = _lib.lib()                               # a build hash that is not the sources', many entry points missing: accepted
    assert loaded.catan_build_hash().decode() != _lib.source_hash() and not hasattr(loaded, missing)
    assert loaded.catan_state_words.restype is _lib._SIGS["catan_state_words"][0]
    with pytest.raises(_lib.CatanHipError):
        _lib.use_library(drv.CPU_LIB)                 # too late: a library is loaded in this process
    assert _lib.lib() is loaded


def test_a_stale_library_is_still_refused_without_use_library(monkeypatch):
    import cpu_abi_driver as drv
    drv.cpu_lib()
    for name in ("_lib", "_foreign", "LIB_PATH"):
        monkeypatch.setattr(_lib, name, getattr(_lib, name))
    monkeypatch.delenv("CATAN_ALLOW_STALE_LIB", raising=False)
    _lib._lib, _lib._foreign, _lib.LIB_PATH = None, False, drv.CPU_LIB
    with pytest.raises(AttributeError):               # bind's default on the normal path
        _lib.lib()
    assert _lib._lib is None


@pytest.mark.parametrize("tool", SEVEN)
def test_help_needs_no_torch(tool):
    p = subprocess.run([sys.executable, "-X", "importtime", os.path.join(TOOLS, tool + ".py"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and b"usage:" in p.stdout
    imported = [ln.rsplit("|", 1)[-1].strip() for ln in p.stderr.decode().splitlines() if ln.startswith("import time:")]
    assert "parent_compare" in imported and "argparse" in imported
    assert not [m for m in imported if m.split(".")[0] in ("torch", "numpy", "settlers_of_catan_rl_amd")]


def test_no_tool_reaches_into_the_binding():
    for tool in SEVEN:
        text = open(os.path.join(TOOLS, tool + ".py")).read()
        for word in ("_lib.LIB_PATH =", "_OPTIONAL", "CATAN_ALLOW_STALE_LIB", "_SYMBOLS", "subprocess", "class UniformRandom",
                     "Event(enable_timing", "step_deferred("):
            if word == "Event(enable_timing" and tool == "bench_playout":
                continue                              # its replica loop puts events around every step of a call: a measurement of its own
            assert word not in text, (tool, word)
        assert "parent_compare" in text
