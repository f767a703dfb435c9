"""Build-time guards on the scene reverb's kernel (kernels_reverb.hip; no GPU needed: hipcc cross-compiles): every build of the
first stage keeps its accumulators in registers, and its loop over the window positions holds the exact-f32 matrix instruction."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openpbso_amd", "csrc")
WIDE_TILES = {1: 8, 2: 8, 3: 4, 4: 4, 5: 2, 6: 2, 7: 2, 8: 2}      # wide_tiles(C) of kernels_reverb.hip; every C also builds one tile


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_reverb_kernel_generated_code(tmp_path):
    out = tmp_path / "kreverb.s"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-S", "--cuda-device-only", os.path.join(CSRC, "kernels_reverb.hip"), "-o", str(out)], check=True, capture_output=True)
    asm = open(out).read()
    code, meta = asm.split(".amdgpu_metadata")[0], asm[asm.find(".amdgpu_metadata"):]
    bodies = {}
    for k in re.split(r"\n(?=_ZN4pbso19scene_reverb_stage1\S*:)", code)[1:]:
        m = re.search(r"scene_reverb_stage1ILi(\d)ELi(\d)EE", k)
        bodies[(int(m.group(1)), int(m.group(2)))] = (m.group(0), k.split("s_endpgm")[0])
    assert set(bodies) == {(c, t) for c in range(1, 9) for t in {1, WIDE_TILES[c]}}
    for (c, t), (name, body) in bodies.items():
        # the loop over the window positions: the innermost loop, from its label to the branch back to it
        loops = [body[m.start():body.find(m.group(1), m.end())] for m in re.finditer(r"\n\.(LBB\d+_\d+):", body)
                 if re.search(r"s_cbranch_\w+ \." + m.group(1) + r"\b", body[m.end():])]
        assert max(len(re.findall(r"\n\s+v_mfma_f32_16x16x4_f32", l)) for l in loops) >= c * t, (c, t)
        assert "scratch_" not in body, (c, t)
        blk = [b for b in meta.split("- .agpr_count") if name in b][0]
        scratch, vgpr, spill, sspill = (int(re.search(r"\.%s:\s+(\d+)" % f, blk).group(1)) for f in
                                        ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count"))
        assert scratch == 0 and spill == 0 and sspill == 0 and vgpr <= 256, (c, t, scratch, vgpr, spill, sspill)
    mfma = set(re.findall(r"\n\s+(v_(?:mfma|smfmac)_\w+)", code))
    assert mfma == {"v_mfma_f32_16x16x4_f32"}, mfma
