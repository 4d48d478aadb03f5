"""The per-atom chain kernels (csrc/tn_chain.hip) keep everything in registers and LDS: the compiler's resource report for
gfx950 must show no scratch memory for any of them (a spill inside the product loops costs more than the fusion gains; the
group-product adjoint was once reverted from a k_tlin9 epilogue for that reason).  Cross-compiles, no GPU needed."""
import os
import re
import subprocess

import __graft_entry__ as ge


def test_chain_kernels_use_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-I" + os.path.join(ge.ROOT, "include"),
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ge.CSRC, "tn_chain.hip"),
           "-o", str(tmp_path / "tn_chain.o")]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    kernels = {}
    name = None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            kernels[name] = int(m.group(1))
        m = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", line)
        if m and name:
            assert int(m.group(1)) >= 2, (name, line)  # two blocks of four waves per CU: one hides the other's stalls
    for key in ("k_chain_readout_fb", "k_chain_gate_fwd", "k_chain_gate_bwd"):
        hit = [n for n in kernels if key in n]
        assert hit, (key, sorted(kernels))
        for n in hit:
            assert kernels[n] == 0, (n, kernels[n])
