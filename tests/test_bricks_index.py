"""The index rule of the brick paging calls (slam-maskrcnn_amd/csrc/semtsdf_bricks.h): a brick is 8
runs of 64 consecutive elements of the tiled layout, element e of run x has place
w = 64 x + 8 ((e >> 2) & 7) + 4 (e >> 5) + (e & 3) in the record.  Expanded per voxel it must equal
tile_index's formula and the real-voxel definition, for every dims triple with x in {8, 11, 24} and
y, z in {8, 12, 28, 32, 40, 72}.  The checker is a stand-alone program built with AddressSanitizer and
UBSan on exact-size heap arrays."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helpers", "bricks_index_check.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_run_and_place_rule_equals_the_per_voxel_definition():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chk")
        subprocess.check_call(["g++", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", exe, SRC])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout, out.stderr[-2000:])
    name, cases, bricks, voxels, bad, real, masked, ragged = out.stdout.split()
    assert name == "bricks"
    assert int(cases) == 3 * 6 * 6
    assert int(bad) == 0, out.stdout
    assert int(voxels) == 512 * int(bricks) and int(real) + int(masked) == int(voxels)
    assert int(real) > 0 and int(masked) > 0 and 0 < int(ragged) < int(bricks)  # both outcomes were exercised
