"""Build-time guards on the kernel of the scene filter mix's delay stage (kernels_fir_delay.hip; no GPU needed: hipcc
cross-compiles), in the manner of tests/test_scene_fir_asm_guards.py: the contraction runs on the exact-f32 matrix instruction
and on no other, no build of it keeps registers in scratch or spills any, and f32 subnormals are kept."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openpbso_amd", "csrc")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_fir_delay_kernel_generated_code(tmp_path):
    out = tmp_path / "kfirdelay.s"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-S", "--cuda-device-only", os.path.join(CSRC, "kernels_fir_delay.hip"), "-o", str(out)], check=True, capture_output=True)
    asm = open(out).read()
    code, meta = asm.split(".amdgpu_metadata")[0], asm[asm.find(".amdgpu_metadata"):]
    bodies = {int(re.search(r"scene_fir_delay_stage1ILi(\d)E", k).group(1)): k.split("s_endpgm")[0]
              for k in re.split(r"\n(?=_ZN4pbso22scene_fir_delay_stage1\S*:)", code)[1:]}
    assert set(bodies) == set(range(1, 9))               # one build per channel count
    for c, body in bodies.items():
        # one accumulator per (channel, tile of 256 samples), two tiles per wave: the loop over the window holds 2 C instructions
        assert len(re.findall(r"\n\s+v_mfma_f32_16x16x4_f32", body)) >= 2 * c, c
        assert "scratch_" not in body, c
        blk = [b for b in meta.split("- .agpr_count") if "scene_fir_delay_stage1ILi%dE" % c in b][0]
        scratch, vgpr, spill, sspill = (int(re.search(r"\.%s:\s+(\d+)" % f, blk).group(1)) for f in
                                        ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count"))
        assert scratch == 0 and spill == 0 and sspill == 0 and vgpr <= 256, (c, scratch, vgpr, spill, sspill)
    assert "scratch_" not in code
    # every matrix instruction of the file is the f32-in / f32-accumulate form: no bf16, f16, xf32, fp8 or scaled one
    mfma = set(re.findall(r"\n\s+(v_(?:mfma|smfmac)_\w+)", code))
    assert mfma == {"v_mfma_f32_16x16x4_f32"}, mfma
    # the read's three operations stay three: nothing of the file is contracted into an f32 fused multiply-add
    assert not re.search(r"\n\s+v_(?:fma|fmac|mad|mac)_f32", code)
    # and no denormal flushing: the kernels run in the default mode, which keeps f32 subnormals
    for blk in re.findall(r"\.amdhsa_kernel .*?\.end_amdhsa_kernel", asm, re.S):
        m = re.search(r"\.amdhsa_float_denorm_mode_32\s+(\d+)", blk)
        assert m is None or int(m.group(1)) == 3
