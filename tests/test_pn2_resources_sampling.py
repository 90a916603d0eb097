"""Compile-time resources of the sampling kernels (no GPU needed). Both register-resident forms live on their register
budget: fps_reg_kernel keeps a point set's coordinates and running distances in registers at four workgroups per CU (1000
hypotheses over 256 CUs need them resident together), and ball_query_reg_kernel keeps the WHOLE point set in every wave's
registers, so a spill would put scratch traffic into loops that are otherwise free of memory waits."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LDS_PER_CU = 160 * 1024
VGPRS_PER_SIMD = 512        # per lane, vector and accumulator halves together
BALL_WAVES = 8              # waves per workgroup of ball_query_reg_kernel (BQR_WAVES)
# workgroups per CU the design record states for each chunk count: two for the sizes the scorer runs (SA2: 512 points =
# 8 chunks, SA1: 2048 points = 32 chunks), one for the 48-chunk form, whose points alone take 144 registers with z
BALL_WORKGROUPS_PER_CU = {8: 2, 16: 2, 32: 2, 48: 1}


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    from ossid_code_amd import _build
    tmp = tmp_path_factory.mktemp("pn2res_sampling")
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
    return res


def _matching(res, pattern):
    """{template argument: resources} of the instantiations whose mangled name matches (the argument is group 1)"""
    hit = {int(m.group(1)): v for k, v in res.items() for m in [re.search(pattern, k)] if m}
    assert hit, sorted(res)
    return hit


def _no_spill(r):
    return r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not installed")
def test_fps_kernels_do_not_spill(resources):
    reg = _matching(resources, r"fps_reg_kernelILi(\d+)E")
    assert sorted(reg) == [2, 4, 8, 12]
    for p, r in reg.items():
        assert _no_spill(r), (p, r)
    lds_form = [v for k, v in resources.items() if re.search(r"\d+fps_kernelE", k)]
    assert len(lds_form) == 1 and _no_spill(lds_form[0]), lds_form
    # the flagship's form: four workgroups of four waves per CU = four waves per SIMD, in registers and in LDS
    # (2048 points x 16 B + 512 picks x 4 B of dynamic LDS beside the static part)
    r = reg[8]
    assert r["Occupancy [waves/SIMD]"] >= 4, r
    assert r["VGPRs"] + r["AGPRs"] <= 128, r
    assert 4 * (r["LDS Size [bytes/block]"] + 2048 * 16 + 512 * 4) <= LDS_PER_CU, r


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not installed")
def test_ball_query_kernels_do_not_spill_and_keep_their_occupancy(resources):
    reg = _matching(resources, r"ball_query_reg_kernelILi(\d+)E")
    assert sorted(reg) == sorted(BALL_WORKGROUPS_PER_CU)
    for nch, r in reg.items():
        assert _no_spill(r), (nch, r)
        wgs = BALL_WORKGROUPS_PER_CU[nch]
        waves_per_simd = wgs * BALL_WAVES // 4
        assert r["Occupancy [waves/SIMD]"] >= waves_per_simd, (nch, r)
        assert (r["VGPRs"] + r["AGPRs"]) * waves_per_simd <= VGPRS_PER_SIMD, (nch, r)
        # all of its LDS is static: three coordinate planes of 64 * nch floats and a row of 320 ints per wave
        assert r["LDS Size [bytes/block]"] >= 64 * nch * 12 + BALL_WAVES * 320 * 4, (nch, r)
        assert wgs * r["LDS Size [bytes/block]"] <= LDS_PER_CU, (nch, r)
    lds_form = [v for k, v in resources.items() if re.search(r"\d+ball_query_kernelE", k)]
    assert len(lds_form) == 1 and _no_spill(lds_form[0]), lds_form
