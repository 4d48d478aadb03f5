"""The fused tensor linears (csrc/tn_tlin9.hip) sit at the 256-register ceiling of two waves per SIMD: the compiler's resource
report for gfx950 must show, for every k_tlin9<PRO, EPI> instance launch_tlin9 can reach, no scratch memory (a reload inside the
double-chunk loops is a vector-memory operation and queues in vmcnt order with the input and weight requests; the update adjoint
<2, 0> once carried 76 bytes per lane), two waves per SIMD and no more than the four chunk buffers of LDS.
Cross-compiles, no GPU needed."""
import os
import re
import subprocess

import __graft_entry__ as ge

# (PRO, EPI) of launch_tlin9: norm, plain, gate, update, update adjoint, norm adjoint, norm + gate adjoint, embedding adjoint
INSTANCES = [(1, 0), (0, 0), (0, 1), (0, 2), (2, 0), (0, 3), (0, 4), (0, 5)]
LDS_MAX = 4 * 3 * 9 * 32 * 32  # four chunk buffers of three bf16 planes of [288 rows][16 k]: 110 592 B


def test_tlin9_instances_fit_two_waves_without_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-I" + os.path.join(ge.ROOT, "include"),
           "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ge.CSRC, "tn_tlin9.hip"),
           "-o", str(tmp_path / "tn_tlin9.o")]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    report = {}
    name = None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            report[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                report[name][key] = int(m.group(1))
    assert LDS_MAX == 110592
    bad = []
    for pro, epi in INSTANCES:
        hit = [n for n in report if f"k_tlin9ILi{pro}ELi{epi}E" in n]
        assert len(hit) == 1, ((pro, epi), sorted(report))
        r = report[hit[0]]
        print((pro, epi), r)
        if not (r["scratch"] == 0 and r["occupancy"] >= 2 and r["lds"] <= LDS_MAX):
            bad.append(((pro, epi), r))
    assert not bad, bad  # every instance is looked at before the verdict: the message names all that are over
