"""The register budget of the 13-bit gate/up launch with unconditional item requests (k_gemm_w13<EPI_SILU, *>,
csrc/gemm_skinny.hip "UNC"): both items' buffers and the launch's activation fragments fit a 1024-thread workgroup — at
most 128 VGPRs, nothing in scratch — and the head of the launch arguments is still preloaded.  Kernel metadata only;
nothing else about the instruction stream is read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dflash_amd", "csrc")
# Itanium mangling of k_gemm_w13<1 /* EPI_SILU */, false> and <1, true>
CHANGED = ["10k_gemm_w13ILi1ELb0EE", "10k_gemm_w13ILi1ELb1EE"]


def _metadata(tmp_path):
    """{mangled kernel name: {directive: value}} of gemm_skinny.hip's .amdhsa_kernel blocks, at build.py's flags."""
    from dflash_amd.build import FLAGS, _hipcc
    hipcc = _hipcc()
    if not (os.path.isabs(hipcc) and os.path.exists(hipcc)) and shutil.which(hipcc) is None:
        pytest.skip("hipcc not found")
    out = os.path.join(str(tmp_path), "gemm_skinny.s")
    subprocess.run([hipcc, *FLAGS, "--cuda-device-only", "-S", os.path.join(CSRC, "gemm_skinny.hip"), "-o", out], check=True,
                   capture_output=True)
    meta, name = {}, None
    for line in open(out):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            name = m.group(1)
            meta[name] = {}
            continue
        if ".end_amdhsa_kernel" in line:
            name = None
        m = re.match(r"\s*\.amdhsa_(\w+)\s+(\d+)", line)
        if m and name:
            meta[name][m.group(1)] = int(m.group(2))
    return meta


def test_unconditional_request_kernels_fit_the_workgroup(tmp_path):
    meta = _metadata(tmp_path)
    for tag in CHANGED:
        hits = [k for k in meta if tag in k]
        assert len(hits) == 1, (tag, sorted(meta))
        d = meta[hits[0]]
        assert d["private_segment_fixed_size"] == 0, (tag, d)
        assert d["next_free_vgpr"] <= 128, (tag, d["next_free_vgpr"])
        assert d.get("user_sgpr_kernarg_preload_length", 0) == 14, (tag, d)
