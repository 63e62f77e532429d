"""The kernel's own rule code on the CPU: csrc/catan_state_check.h, the lines k_state_check compiles, built for the host with the
undefined-behaviour and address sanitizers (tools/native/state_check_host.cpp, a stand-alone program) and run over legal blobs, every
planted corruption and the 3 680 single-word corruptions of the totality test.  The masks are the numpy reference's, whole words, and a
shift by an unchecked word, an index past an array or a signed overflow would end the run."""
import os
import subprocess

import numpy as np
import pytest

import state_check_cases as cases
import state_check_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("state_check_host")
    exe = str(d / "state_check_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-w", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "settlers_of_catan_rl_amd", "csrc"), os.path.join(ROOT, "tools", "native", "state_check_host.cpp"), "-o", exe],
                   check=True)

    def run(blobs):
        np.ascontiguousarray(blobs, dtype=np.int32).tofile(str(d / "in.bin"))
        r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        return np.fromfile(str(d / "out.bin"), dtype=np.uint64)
    return run


def test_host_build_of_the_kernel_rules_equals_the_reference(oracle, host_check):
    planted = cases.planted()
    blobs = np.concatenate([cases.legal_pool(), np.array([b for _, b, _ in planted]), cases.finals()])
    got = host_check(blobs)
    assert np.array_equal(got, ref.state_check(blobs))
    assert not got[:512].any() and [int(g) for g in got[512:512 + len(planted)]] == [cases.expected_mask(r) for _, _, r in planted]


def test_host_build_is_total_on_single_word_corruptions(oracle, host_check):
    blobs = cases.totality_blobs()
    got, want = host_check(blobs), ref.state_check(blobs)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, [(int(i) // 5, cases.TOTALITY_VALUES[int(i) % 5], ref.explain(got[i]), ref.explain(want[i])) for i in bad[:6]]


def test_host_build_takes_whole_blobs_of_extreme_words(oracle, host_check):
    """every word at once at each extreme, and random int32 noise: still the reference's masks"""
    rng = np.random.default_rng(5)
    blobs = np.concatenate([np.full((1, 736), v, dtype=np.int64) for v in cases.TOTALITY_VALUES + (0, 1, 4, 25)]
                           + [rng.integers(-2 ** 31, 2 ** 31, size=(64, 736)), rng.integers(-2, 8, size=(256, 736))]).astype(np.int32)
    assert np.array_equal(host_check(blobs), ref.state_check(blobs))
