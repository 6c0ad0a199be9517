"""CPU suite: the per-episode kernels compiled for the reference shape (csrc/episode.hip, query_lds_kernel<true, true, DROP> and
reverse_lds_kernel<true, DROP>) build for gfx950 without scratch memory and without SGPR spills.  The run-time-shaped forms they
replace spill 60+ / 220+ SGPRs; the fixed forms exist to remove that scalar work, so a spill coming back is a regression."""
import os
import re
import subprocess

from conftest import ROOT


def test_fixed_shape_episode_kernels_use_no_scratch(tmp_path):
    src = os.path.join(ROOT, "fumi_amd", "csrc", "episode.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-Os", "-std=c++17", "-fPIC", "-c", src, "-o", str(tmp_path / "o.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    name, seen = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen[name] = {}
        m = re.search(r"(ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill): (\d+)", line)
        if m and name:
            seen[name][m.group(1)] = int(m.group(2))
    # mangled: query_lds_kernelILb1ELb1ELb{0,1}E, reverse_lds_kernelILb1ELb{0,1}E
    fixed = {k: v for k, v in seen.items() if re.search(r"query_lds_kernelILb1ELb1ELb[01]E|reverse_lds_kernelILb1ELb[01]E", k)}
    assert len(fixed) == 4, sorted(seen)
    for k, v in fixed.items():
        assert v.get("ScratchSize [bytes/lane]") == 0 and v.get("VGPRs Spill") == 0 and v.get("SGPRs Spill") == 0, (k, v)
