"""Register budget of the GroupNorm kernels (csrc/norm.hip), read from hipcc's resource remarks: the streaming kernels hide memory
latency with resident waves, so an instantiation that spills, or that needs more registers than five waves per SIMD allow, is a
regression no output check notices."""
import os
import re
import shutil
import subprocess

import pytest

VGPR_BOUND = 96       # 512 VGPRs per SIMD lane / 5 waves, in the allocation granule of 8
SIXTEEN_BIT = {"1", "6"}     # MF_BF16, MF_F16 (include/mfhip.h)


def test_16_bit_groupnorm_kernels_keep_five_waves_per_simd_and_no_scratch(tmp_path):
    """Every gn_apply_kernel and gn_slab_kernel instantiation that reads and writes 16-bit storage (the flavours a bf16 / fp16 step
    runs; an fp32 row takes twice the registers per row in flight and is not held to this) compiles for gfx950 with 0 bytes of
    scratch and at most 96 VGPRs."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    from reflecting_reality_amd import _build
    res = subprocess.run([hipcc, *_build.HIPCC_FLAGS, "--cuda-device-only", "-c", os.path.join(_build.CSRC, "norm.hip"),
                          "-o", str(tmp_path / "n.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    seen = {"gn_apply_kernel": 0, "gn_slab_kernel": 0}
    for block in res.stderr.split("Function Name: ")[1:]:
        name = block.split()[0]
        m = re.search(r"\d+(gn_apply_kernel|gn_slab_kernel)ILi(\d+)ELi(\d+)E", name)
        if not m or m.group(2) not in SIXTEEN_BIT or m.group(3) not in SIXTEEN_BIT:
            continue
        info = {k: int(v) for k, v in re.findall(r"remark:\s+([\w ]+?)(?: \[[\w/]+\])?: (\d+) \[", block)}
        print(f"{name}: VGPRs {info['VGPRs']}, scratch {info['ScratchSize']}, spilled VGPRs {info['VGPRs Spill']}, "
              f"waves/SIMD {info['Occupancy']}")
        assert info["ScratchSize"] == 0 and info["VGPRs Spill"] == 0, f"{name} spills: {info}"
        assert info["VGPRs"] <= VGPR_BOUND, f"{name} needs {info['VGPRs']} VGPRs"
        seen[m.group(1)] += 1
    # bf16 and fp16, SiLU on / off: two vector widths x one / two segments of the apply kernel (four rows in flight are a constant of
    # the kernel, no longer a template argument with an 8-row flavour beside it), the slab kernel with and without a deferred split-K input
    assert seen == {"gn_apply_kernel": 16, "gn_slab_kernel": 8}, seen
