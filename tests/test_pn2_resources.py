"""Compile-time resources of the SA1 kernel (no GPU needed): it holds its three weight layers in registers at one wave per
SIMD, which only works while nothing spills -- a spilled weight quad is a scratch load in the middle of the MFMA stream."""
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


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not installed")
def test_sa1_kernel_has_no_scratch(tmp_path):
    from ossid_code_amd import _build
    src = os.path.join(_build.CSRC, "pn2.hip")
    cmd = [_hipcc()] + _build.FLAGS + _build.SOURCE_FLAGS.get("pn2.hip", []) + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                                       str(tmp_path / "pn2.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    res = {}
    for b in blocks:
        name = b.split()[0]
        res[name] = {k: int(v) for k, v in re.findall(r"remark: [^\n]*?\s(ScratchSize \[bytes/lane\]|VGPRs|AGPRs|VGPRs Spill|"
                                                      r"Occupancy \[waves/SIMD\]): (\d+)", b)}
    sa1 = [v for k, v in res.items() if "sa1_kernel" in k]
    assert len(sa1) == 1, sorted(res)
    sa1 = sa1[0]
    assert sa1["ScratchSize [bytes/lane]"] == 0 and sa1["VGPRs Spill"] == 0, sa1
    assert sa1["VGPRs"] + sa1["AGPRs"] <= 512 and sa1["Occupancy [waves/SIMD]"] == 1, sa1
