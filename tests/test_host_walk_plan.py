"""The backward's band plan in its cost-ordered, cost-balanced form (plan_bands with an order, sparkfm_amd/csrc/fmhip_host.cpp):
a stand-alone program under AddressSanitizer and UBSan, in the style of the host arithmetic harness.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walk_plan_invariants_under_the_sanitizers(tmp_path):
    """tests/host_walk_plan.cpp over seeded random transposes, for the stream order and cold-first: every range
    exactly once across the eight lists in the interval form and in the walk form, both forms of a list the same ranges, every
    run of the interval form ascending (feature-interval launches clip the runs by binary search), the free part of the walk
    form whole blocks of 32 in non-increasing cost, and the lists' accumulated costs within one block's cost of each other."""
    exe = str(tmp_path / "host_walk_plan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           os.path.join(ROOT, "tests", "host_walk_plan.cpp"), os.path.join(ROOT, "sparkfm_amd", "csrc", "fmhip_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("no sanitizer runtime for g++ in this image")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    env.pop("FMHIP_ROW_BANDS", None)
    for seed in (20261018, 3):
        r = subprocess.run([exe, str(seed), "12"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
        assert r.returncode == 0 and b"checks ok" in r.stdout, (seed, r.stderr.decode()[-3000:])
