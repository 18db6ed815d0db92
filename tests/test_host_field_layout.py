"""The field models' slot maps (sparkfm_amd/csrc/fmhip_field_layout.h: where FwFM's r, FmFM's MM and the dense array of DeepFM, DCN and
AutoInt keep the caller's elements) in tests/host_field_layout_harness.cpp, a stand-alone program under ASan and UBSan: no GPU, and not
the library loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("field_layout") / "host_field_layout_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "host_field_layout_harness.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("no sanitizer runtime for g++ in this image")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r.stdout.decode().splitlines()


@pytest.mark.parametrize("model,cases", [("fwfm", 4), ("fmfm", 4), ("deepfm", 8), ("dcn", 8), ("autoint", 16)])
def test_slot_maps_under_the_sanitizers(lines, model, cases):
    """F = 1 and 17 (Fp and Pp differ from F and F Kp), k = 1 and 5 (Kp = 4 and 8), one layer and three, DCN at rank 16, AutoInt at
    1 and 4 heads of 16, DeepFM with widths 32, 16, 48."""
    mine = [l for l in lines if l.startswith("ok %s " % model)]
    assert len(mine) == cases, lines
    assert all(int(l.split()[-3]) <= int(l.split()[-1]) for l in mine)          # slots <= total


def test_padding_is_exercised(lines):
    """At F = 17, k = 5 every map but FwFM's has device slots no caller slot maps to."""
    for model in ("fmfm", "deepfm", "dcn", "autoint"):
        wide = [l.split() for l in lines if l.startswith("ok %s F 17 k 5" % model)]
        assert wide and all(int(w[-3]) < int(w[-1]) for w in wide), model
