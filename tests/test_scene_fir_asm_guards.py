"""Build-time guards on the kernels of the scene filter mix (kernels_fir.hip; no GPU needed: hipcc cross-compiles).  The first
stage is one kernel template built for four variants -- plain, behind the delay stage, with scheduled sets, and both -- and
every build of each variant is held to the same: the contraction runs on the exact-f32 matrix instruction and on no other, no
build keeps registers in scratch or spills any.  For the whole file: nothing is contracted into an f32 fused multiply-add (the
read of the delay stage and a fade's blend are three separately rounded operations), and f32 subnormals are kept."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openpbso_amd", "csrc")

# variant -> (its argument struct in the kernel's mangled name, the builds there must be)
VARIANTS = {
    "plain": (r"scene_fir_stage1ILi(\d)ENS_8FirPlainE", {(c,) for c in range(1, 9)}),
    "delay": (r"scene_fir_stage1ILi(\d)ENS_8FirDelayE", {(c,) for c in range(1, 9)}),
    "sched": (r"scene_fir_stage1ILi(\d)ENS_8FirSchedILb([01])EEE", {(c, d) for c in range(1, 9) for d in (0, 1)}),
}
N_OTHER_KERNELS = 7      # prepare, delay expand, both second stages, the history kernel, both z-history kernels


@pytest.fixture(scope="module")
def fir_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("kfir") / "kfir.s"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-S", "--cuda-device-only", os.path.join(CSRC, "kernels_fir.hip"), "-o", str(out)], check=True, capture_output=True)
    return open(out).read()


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_fir_kernel_generated_code(fir_asm, variant):
    asm = fir_asm
    pattern, builds = VARIANTS[variant]
    code, meta = asm.split(".amdgpu_metadata")[0], asm[asm.find(".amdgpu_metadata"):]
    bodies = {tuple(int(g) for g in m.groups()): k.split("s_endpgm")[0]
              for k in re.split(r"\n(?=_ZN4pbso16scene_fir_stage1\S*:)", code)[1:]
              for m in [re.search(pattern, k.split(":")[0])] if m}
    assert set(bodies) == builds                         # one build per channel count (sched: with and without the delay stage)
    blocks = meta.split("- .agpr_count")[1:]
    for key, body in bodies.items():
        # one accumulator per (channel, tile of 256 samples), two tiles per wave: the loop over the window holds 2 C instructions
        assert len(re.findall(r"\n\s+v_mfma_f32_16x16x4_f32", body)) >= 2 * key[0], key
        assert "scratch_" not in body, key
        blk = [b for b in blocks if re.search(pattern, b) and tuple(int(g) for g in re.search(pattern, b).groups()) == key][0]
        scratch, vgpr, spill, sspill = (int(re.search(r"\.%s:\s+(\d+)" % f, blk).group(1)) for f in
                                        ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count"))
        assert scratch == 0 and spill == 0 and sspill == 0 and vgpr <= 256, (key, scratch, vgpr, spill, sspill)
    # every kernel of the file: no scratch, no VGPR or SGPR spills
    assert len(blocks) == sum(len(b) for _, b in VARIANTS.values()) + N_OTHER_KERNELS
    for blk in blocks:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        scratch, vgpr, spill, sspill = (int(re.search(r"\.%s:\s+(\d+)" % f, blk).group(1)) for f in
                                        ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count"))
        assert scratch == 0 and spill == 0 and sspill == 0 and vgpr <= 256, (name, scratch, vgpr, spill, sspill)
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
