"""Build-time guard on what K1b (kernels_block.hip) spends on its vector ALU BETWEEN two buffers' matrix pipelines (no GPU needed:
hipcc cross-compiles; the compile line of tests/test_kernel_asm_guards.py, the R = 4 builds only).  Vector and matrix instructions
share one datapath on gfx950, so every vector instruction of a buffer's head, combine and prefetches is taken from the SIMD partner's
MFMAs (profiles/k1b_between_pipelines.txt).  In the buffer loop of the headline build <R = 4, qnorm rows, f32 projection>:
  - the per-lane loads and stores go through an SGPR base + a 32-bit lane offset: the 64-bit vector address operations left are
    those of the explicit-data force-gain row (a slow path: 4 per copy of the prefetch);
  - scalars parked in VGPR lanes are read back on slow paths only (the transfer-row change, the LDS-DMA of a direct hit, a skipped
    buffer) and for the combine's store base; the four v_readlane_b32 of every wave sum are counted too.
The counts are the ones the code reached, with a little slack for the compiler; the registers must not grow."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openpbso_amd", "csrc")
HEADLINE = "ILi4ELi2ELi0ELb0ELi512ELb0ELb0E"
READLANE_MAX, ADDR64_MAX = 44, 16          # reached: 40 and 12


def buffer_loop(body):
    """the lines of the basic blocks that belong to the loop around the MFMAs (the loop over a launch's buffers), by the compiler's
    own loop comments on the block labels"""
    lines = body.splitlines()
    first_mfma = next(i for i, l in enumerate(lines) if "v_mfma" in l)
    lab = max(i for i, l in enumerate(lines[:first_mfma]) if re.match(r"\.LBB\d+_\d+:", l))
    m = re.search(r"Header=(BB\d+_\d+) Depth=1", lines[lab])
    hdr = m.group(1) if m else lines[lab].split(":")[0][2:]
    inside, cur = [], False
    for l in lines:
        if re.match(r"\.LBB\d+_\d+:", l):
            cur = l.startswith(".L" + hdr + ":") or ("Header=" + hdr + " ") in l or ("Parent Loop " + hdr + " ") in l
        if cur:
            inside.append(l)
    return inside


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not available")
def test_headline_buffer_loop_vector_overhead(tmp_path):
    out = tmp_path / "kb.s"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-DPBSO_ONLY_R4",
                    "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                    os.path.join(CSRC, "kernels_block.hip"), "-o", str(out)], check=True, capture_output=True)
    asm = open(out).read()
    bodies = [k for k in re.split(r"\n(?=_ZN4pbso9iir_block16iir_block_kernel\S*:)", asm)[1:] if k.startswith("_ZN4pbso9iir_block16iir_block_kernel" + HEADLINE)]
    assert len(bodies) == 1
    loop = buffer_loop(bodies[0].split("s_endpgm")[0])
    assert sum(1 for l in loop if re.match(r"\s+v_mfma_f32_16x16x4_f32\b", l)) == 256          # it IS the buffer loop
    n_readlane = sum(1 for l in loop if re.match(r"\s+v_readlane_b32\b", l))
    n_addr64 = sum(1 for l in loop if re.match(r"\s+v_(lshlrev_b64|lshl_add_u64)\b", l))
    # the parent of this change: 63 and 138 in the loop's body as the issue counted them (51 and 121 by the blocks counted here)
    assert n_readlane <= READLANE_MAX < 51 < 63, n_readlane
    assert n_addr64 <= ADDR64_MAX < 121 < 138, n_addr64
    meta = asm[asm.find(".amdgpu_metadata"):]
    m = re.search(r"\.name:\s+_ZN4pbso9iir_block16iir_block_kernel" + HEADLINE + r".*?\.sgpr_count:\s+(\d+).*?\.vgpr_count:\s+(\d+)", meta, re.S)
    sgprs, vgprs = int(m.group(1)), int(m.group(2))
    assert sgprs <= 106 and vgprs <= 253, (sgprs, vgprs)          # the parent's
