"""The workspace plans of libppfit's chunked entry points (csrc/ppfit_wsplan.hpp).

tools/ws_plan_check.cpp is a host program: it declares the arrays of each of
the eight chunked sites the way the library's host files do and compares the
chunk, every array's offset and the total against literal numbers from the
hand-written arithmetic the planner replaced -- at workspace limits that give
one item per chunk, three (from both ends of the divisor's range), all of
them, and the 65535-item cap.  Built with the host compiler and run here; no
GPU.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ws_plans(tmp_path):
    exe = str(tmp_path / "ws_plan_check")
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "pulseportraiture_amd", "csrc"),
                           os.path.join(ROOT, "tools", "ws_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "ok"
