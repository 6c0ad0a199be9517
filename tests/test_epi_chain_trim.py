"""The layout constants that the fixed-address staging of reverse_lds_kernel<true, DROP> relies on are `static_assert`s in
csrc/episode.hip (`ref_rlay_ok()`: 16-byte image offsets, the row stride of the 64-column images, the arena's size; one lane per
staged float4).  They are checked when the file is compiled, so a cross-compile for gfx950 is the test on a machine without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "fumi_amd", "csrc", "episode.hip")


def test_reference_layout_asserts_hold_for_gfx950():
    text = open(SRC).read()
    assert "static_assert(ref_rlay_ok()" in text and "constexpr bool ref_rlay_ok()" in text
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", SRC], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "static assertion failed" not in r.stderr
