"""The carving helper of the handle's device buffers (wb_humanoid_mpc_amd/csrc/hsqp_carve.h) is plain C++: tests/carve/carve_check.cpp is built with the
host compiler under the address and undefined-behaviour sanitizers and run as a program of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_carve_check_under_sanitizers(tmp_path):
    exe = tmp_path / "carve_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "wb_humanoid_mpc_amd", "csrc"), os.path.join(ROOT, "tests", "carve", "carve_check.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True)
    assert out.strip() == "carve ok"
