"""The index maps of k_post_w (csrc/ppfit_vthread.hpp) against the block's.

tools/post_wave_map_check.cpp is a host program: for every count of fitted
channels 1..80 (and beyond a block's stride) it walks the per-thread channel
loops and the with-scales sweep of the 256-thread post-fit and of the one-wave
kernel with the helpers the kernels use, and compares which operands each sum
adds and in which order.  Built with the host compiler and run here; no GPU.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_post_wave_maps(tmp_path):
    exe = str(tmp_path / "post_wave_map_check")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "pulseportraiture_amd", "csrc"),
                           os.path.join(ROOT, "tools", "post_wave_map_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "ok"
