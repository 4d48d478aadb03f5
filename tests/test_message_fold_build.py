"""The tile sweeps (csrc/tn_message_pair.hip).  The reverse ones - k_message_adjoint_rows8 and k_message_adjoint_rows8_fold, which
computes the group-product adjoint in its prologue - live at the edge of the register file: 240 VGPRs in the edge loop, two waves
per SIMD.  The compiler's resource report for gfx950 must show no scratch memory and an occupancy of at least 2 for every one of
them - the same algebra spilled as a k_tlin9 epilogue and lost to the pair of launches it replaced.  The forward sweep
k_message_rows8<8, 4> shares its prologue, walk and accumulation with them (force-inlined helpers that take the accumulators as
references to arrays) and is held to the same two conditions.  Cross-compiles, no GPU needed."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as ge


@pytest.fixture(scope="module")
def resource_report(tmp_path_factory):
    """kernel name (mangled) -> scratch bytes per lane, and -> waves per SIMD, of one compilation of the file"""
    tmp_path = tmp_path_factory.mktemp("tn_message_pair")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-I" + os.path.join(ge.ROOT, "include"),
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ge.CSRC, "tn_message_pair.hip"),
           "-o", str(tmp_path / "tn_message_pair.o")]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    scratch, occupancy = {}, {}
    name = None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
        m = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", line)
        if m and name:
            occupancy[name] = int(m.group(1))
    return scratch, occupancy


def test_adjoint_tile_sweeps_use_no_scratch(resource_report):
    scratch, occupancy = resource_report
    hit = sorted(n for n in scratch if "k_message_adjoint_rows8" in n)
    assert len(hit) == 2 and any("k_message_adjoint_rows8_fold" in n for n in hit), (hit, sorted(scratch))
    for n in hit:
        assert scratch[n] == 0, (n, scratch[n])
        assert occupancy[n] >= 2, (n, occupancy[n])


def test_forward_tile_sweep_uses_no_scratch(resource_report):
    scratch, occupancy = resource_report
    hit = sorted(n for n in scratch if "k_message_rows8ILi8ELi4E" in n)  # k_message_rows8<8, 4>
    assert len(hit) == 1, (hit, sorted(scratch))
    assert scratch[hit[0]] == 0, (hit[0], scratch[hit[0]])
    assert occupancy[hit[0]] >= 2, (hit[0], occupancy[hit[0]])
