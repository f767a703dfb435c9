"""Build-time guards on the kernels of the scene filter mix's schedule (kernels_fir_sched.hip; no GPU needed: hipcc cross-compiles),
in the manner of tests/test_scene_fir_delay_asm_guards.py, for that file only: the contraction runs on the exact-f32 matrix
instruction and on no other, no build keeps registers in scratch or spills any, nothing is contracted into an f32 fused
multiply-add, and f32 subnormals are kept."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openpbso_amd", "csrc")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_fir_sched_kernels_generated_code(tmp_path):
    out = tmp_path / "kfirsched.s"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-S", "--cuda-device-only", os.path.join(CSRC, "kernels_fir_sched.hip"), "-o", str(out)], check=True, capture_output=True)
    asm = open(out).read()
    code, meta = asm.split(".amdgpu_metadata")[0], asm[asm.find(".amdgpu_metadata"):]
    bodies = {(int(m.group(1)), int(m.group(2))): k.split("s_endpgm")[0]
              for k in re.split(r"\n(?=_ZN4pbso22scene_fir_sched_stage1\S*:)", code)[1:]
              for m in [re.search(r"scene_fir_sched_stage1ILi(\d)ELb([01])E", k)]}
    assert set(bodies) == {(c, d) for c in range(1, 9) for d in (0, 1)}      # one build per channel count, with and without the delay stage
    for (c, d), body in bodies.items():
        assert len(re.findall(r"\n\s+v_mfma_f32_16x16x4_f32", body)) >= 2 * c, (c, d)
        assert "scratch_" not in body, (c, d)
    # every kernel of the file: no scratch, no VGPR or SGPR spills
    blocks = [b for b in meta.split("- .agpr_count")[1:]]
    assert len(blocks) == 16 + 4
    for blk in blocks:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        scratch, vgpr, spill, sspill = (int(re.search(r"\.%s:\s+(\d+)" % f, blk).group(1)) for f in
                                        ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count"))
        assert scratch == 0 and spill == 0 and sspill == 0 and vgpr <= 256, (name, scratch, vgpr, spill, sspill)
    assert "scratch_" not in code
    mfma = set(re.findall(r"\n\s+(v_(?:mfma|smfmac)_\w+)", code))
    assert mfma == {"v_mfma_f32_16x16x4_f32"}, mfma
    assert not re.search(r"\n\s+v_(?:fma|fmac|mad|mac)_f32", code)
    for blk in re.findall(r"\.amdhsa_kernel .*?\.end_amdhsa_kernel", asm, re.S):
        m = re.search(r"\.amdhsa_float_denorm_mode_32\s+(\d+)", blk)
        assert m is None or int(m.group(1)) == 3
