"""The arithmetic that cuts the persistent SA kernels' work-balanced slices (csrc/slice_balance.h, SPEC 4.5), checked on the
CPU (no GPU needed): tools/slice_balance_check.cpp is a stand-alone program built with -fsanitize=address,undefined that
shows, for random and adversarial hit counts, that the slices tile [0, total) exactly and in order, that each boundary is
where a brute-force scan puts it, and that no slice costs more than W / nw plus one centre plus the targets' rounding. A
boundary outside [0, total] would be an out-of-bounds gather in sa1_kernel / sa2_kernel."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cxx():
    for cand in ("g++", "clang++", "c++"):
        if shutil.which(cand):
            return shutil.which(cand)
    return None


@pytest.mark.skipif(_cxx() is None, reason="no host C++ compiler")
def test_slices_tile_the_centres_under_sanitizers(tmp_path):
    exe = str(tmp_path / "slice_balance_check")
    cmd = [_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tools", "slice_balance_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    assert "slice_balance_check: ok" in r.stderr and "ERROR" not in r.stderr, r.stderr[-1500:]
    assert "total < nw" in r.stdout and "costs of 1 only" in r.stdout and "one hypothesis" in r.stdout, r.stdout[-1500:]
