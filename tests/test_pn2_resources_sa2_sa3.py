"""Compile-time resources of the SA2 and SA3 kernels (no GPU needed). sa2_kernel holds its middle layer in the accumulator
half of the register file and its last layer in LDS at one wave per SIMD: a spilled weight quad would be a scratch load in
the middle of the MFMA stream, and an LDS image over 160 KiB would not launch. sa3_kernel must not spill either."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    from ossid_code_amd import _build
    tmp = tmp_path_factory.mktemp("pn2res")
    src = os.path.join(_build.CSRC, "pn2.hip")
    cmd = [_hipcc()] + _build.FLAGS + _build.SOURCE_FLAGS.get("pn2.hip", []) + \
        ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp / "pn2.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp))
    assert r.returncode == 0, r.stderr[-2000:]
    res = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
        res[b.split()[0]] = {k: int(v) for k, v in re.findall(
            r"remark: [^\n]*?\s(ScratchSize \[bytes/lane\]|VGPRs|AGPRs|VGPRs Spill|SGPRs Spill|Occupancy \[waves/SIMD\]|"
            r"LDS Size \[bytes/block\]): (\d+)", b)}
    return res, src


def _one(res, kernel):
    hit = [v for k, v in res.items() if kernel in k]
    assert len(hit) == 1, sorted(res)
    return hit[0]


def _static_lds_floats(src):
    """sa2_kernel's LDS is dynamic (the compiler reports 0): its size is the SA2_LDS_FLOATS constant the launcher passes."""
    text = open(src).read()
    m = re.search(r"constexpr int ([^;]*SA2_LDS_FLOATS[^;]*);", text)
    assert m, "SA2_LDS_FLOATS not found"
    env = {}
    for name, expr in re.findall(r"(\w+)\s*=\s*([^,;]+)", m.group(1)):
        env[name] = int(eval(expr, {"__builtins__": {}}, env))
    return env["SA2_LDS_FLOATS"]


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not installed")
def test_sa2_kernel_resources(resources):
    res, src = resources
    sa2 = _one(res, "sa2_kernel")
    assert sa2["ScratchSize [bytes/lane]"] == 0 and sa2["VGPRs Spill"] == 0 and sa2["SGPRs Spill"] == 0, sa2
    assert sa2["VGPRs"] + sa2["AGPRs"] <= 512, sa2
    assert sa2["Occupancy [waves/SIMD]"] == 1, sa2
    lds = sa2["LDS Size [bytes/block]"] + 4 * _static_lds_floats(src)
    assert 0 < lds <= 160 * 1024, lds


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not installed")
def test_sa3_kernel_has_no_scratch(resources):
    res, _ = resources
    sa3 = _one(res, "sa3_kernel")
    assert sa3["ScratchSize [bytes/lane]"] == 0 and sa3["VGPRs Spill"] == 0 and sa3["SGPRs Spill"] == 0, sa3
