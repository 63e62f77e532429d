"""Which branches of the oracle's rule code do the reference-recorded fixtures reach?

The HIP environment is held to the CPU oracle bit for bit; the oracle is held to the reference only through the recorded data under
tests/golden/.  A rule branch that data never takes is a place where kernel and oracle can agree and both misread the reference.
This test builds oracle/catan_oracle.c with `-O0 --coverage`, runs the reference-derived tests of test_oracle_golden.py against that
library in a child process, reads `gcov --json-format`, and asserts that inside the rule functions the set of never-taken branches
EQUALS the committed allow-list (tests/rule_coverage_allowlist.py), both ways: a branch that is no longer reached fails (a fixture
lost its case, or new rule code came without reference data), and an allow-listed branch that is reached fails too (a stale entry).

Host only: plain gcc and gcov, nothing preloaded, no GPU."""
import gzip
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

import rule_coverage_allowlist as allow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "oracle", "catan_oracle.c")
CFLAGS = ["-O0", "--coverage", "-fPIC", "-std=c11", "-fopenmp"]
# the tests of test_oracle_golden.py whose expected values the reference produced
CHILD_TESTS = "test_trajectory or test_validate_cases or test_mt19937_known_answer or test_reset_states or " \
              "test_randomise_uncertainty_golden or test_longest_road_cases"
RULE_FUNCTIONS = re.compile(r"^(update_estimates\w*|update_longest_road|update_largest_army|can_place_\w+|valid_roads|valid_dev_cards|"
                            r"orc_masks|roll_dice|update_players_go|orc_step|player_inputs|orc_obs)$")


def _find_gcov():
    """the gcov of the installed gcc: `gcov-<major>` first (its data format follows the compiler's version), then plain `gcov`"""
    major = subprocess.run(["gcc", "-dumpversion"], capture_output=True, text=True).stdout.strip().split(".")[0]
    for name in (f"gcov-{major}", "gcov"):
        path = shutil.which(name)
        if path:
            return path
    return None


def never_taken(gcov_json, source_lines):
    """-> {(function, stripped line text, occurrence of that text within the function, branch index)} of the rule functions' branches
    with count 0.  Keyed by text, not by line number, so that unrelated edits of the file leave the allow-list valid."""
    (f,) = [x for x in gcov_json["files"] if os.path.basename(x["file"]) == "catan_oracle.c"]
    seen, out, total = {}, set(), 0
    for ln in sorted(f["lines"], key=lambda x: x["line_number"]):
        fn = ln.get("function_name", "")
        if not ln["branches"] or not RULE_FUNCTIONS.match(fn):
            continue
        text = source_lines[ln["line_number"] - 1].strip()
        k = seen[(fn, text)] = seen.get((fn, text), -1) + 1
        for i, b in enumerate(ln["branches"]):
            total += 1
            if b["count"] == 0:
                out.add((fn, text, k, i))
    return out, total


def _fmt(keys):
    return "\n".join(f"  {fn}: `{text}` (occurrence {k}) branch {i}" for fn, text, k, i in sorted(keys))


def test_rule_branches_reached_by_reference_fixtures(tmp_path):
    gcov = _find_gcov()
    if shutil.which("gcc") is None or gcov is None:
        pytest.skip("no gcc / gcov on this machine: branch coverage of the oracle cannot be measured")
    obj, lib = tmp_path / "catan_oracle.o", tmp_path / "libcatan_oracle_cov.so"
    subprocess.run(["gcc"] + CFLAGS + ["-c", "-o", str(obj), SRC], check=True, cwd=tmp_path)
    subprocess.run(["gcc"] + CFLAGS + ["-shared", "-o", str(lib), str(obj), "-lm"], check=True, cwd=tmp_path)
    env = dict(os.environ, CATAN_ORACLE_LIB=str(lib), PYTHONDONTWRITEBYTECODE="1")
    env.pop("CATAN_ORACLE_ASAN", None)
    child = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_oracle_golden.py"),
                            "-k", CHILD_TESTS], cwd=ROOT, env=env, capture_output=True, text=True)
    assert child.returncode == 0, child.stdout[-3000:] + child.stderr[-2000:]
    assert (tmp_path / "catan_oracle.gcda").exists(), "the child process did not load the instrumented library"
    subprocess.run([gcov, "-b", "-c", "--json-format", "-o", str(obj), SRC], check=True, cwd=tmp_path, capture_output=True)
    (out,) = list(tmp_path.glob("*.gcov.json.gz"))
    with gzip.open(out, "rt") as fh:
        data = json.load(fh)
    got, total = never_taken(data, open(SRC).read().split("\n"))
    assert total > 500, total                    # the rule functions were found and instrumented
    want = {(fn, text, k, i) for fn, text, k, i, _ in allow.NEVER_TAKEN}
    assert len(want) == len(allow.NEVER_TAKEN), "duplicate allow-list entries"
    assert all(isinstance(r, str) and len(r.strip()) > 10 for *_, r in allow.NEVER_TAKEN), "every entry carries its reason"
    new, stale = got - want, want - got
    assert not new, f"{len(new)} rule branches no reference fixture takes (add reference data that reaches them):\n" + _fmt(new)
    assert not stale, f"{len(stale)} allow-listed branches are reached now (or their line changed): remove them\n" + _fmt(stale)
