"""The camera helpers and staging layouts of the host API (slam-maskrcnn_amd/csrc/semtsdf_cam.h) as a
stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer on the CPU
(tests/helpers/api_parts_check.cpp): the helpers reproduce, bit for bit and to the sign of a zero,
the expressions their call sites held before, for five poses and intrinsics; the maps, tracking and
ray-state layouts have the documented offsets, alignments and totals at 1, 75 x 53 and 640 x 480
pixels, and no two of their arrays overlap."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helpers", "api_parts_check.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_camera_helpers_and_layouts_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chk")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-o", exe, SRC])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = out.stdout.splitlines()
    cameras = [ln.split()[1:] for ln in lines if ln.startswith("camera ")]
    assert cameras == [[n, "ok"] for n in ("identity", "general", "negative-column", "negative-zero-t",
                                           "non-pinhole-K")], out.stdout
    # the one input at which the two forms of the origin part: -0.0f (pose, ICP) and +0.0f (association)
    assert "origin forms at the all-negative column: pose 80000000 assoc 00000000" in lines, out.stdout
    layouts = [ln.split()[1:] for ln in lines if ln.startswith("layout ")]
    assert layouts == [[name, f"n={n}", "ok"] for n in (1, 75 * 53, 640 * 480) for name in ("maps", "tracking", "ray")], \
        out.stdout
    assert lines[-1] == "failures 0", out.stdout
