"""The index rule of semtsdf_shift (slam-maskrcnn_amd/csrc/semtsdf_shift.h): a destination line
of the tiled layout is gathered from one source line or from nothing, with a per-voxel mask on
ragged dims.  Expanded per voxel through tile_index's formula it must equal the definition (voxel
i holds what voxel i + s held, the reset state where there is no source, padding stays reset),
writing every stored index exactly once, for every dims triple in {8, 11, 24} x {8, 13, 28} x
{32, 37, 72} and every shift with components in {0, +-8, +-16, +-32, +-80}.  The checker is a
stand-alone program built with AddressSanitizer and UBSan on exact-size heap arrays."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helpers", "shift_index_check.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_line_rule_equals_the_per_voxel_definition():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chk")
        subprocess.check_call(["g++", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", exe, SRC])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout, out.stderr[-2000:])
    name, cases, lines, voxels, bad, copied, masked = out.stdout.split()
    assert name == "shift"
    assert int(cases) == 27 * 9 ** 3
    assert int(lines) >= 100_000 and int(bad) == 0, out.stdout
    assert int(voxels) == 32 * int(lines)
    assert int(copied) > 0 and int(masked) > 0  # both outcomes were exercised
