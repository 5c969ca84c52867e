"""The marches' one stepping routine (slam-maskrcnn_amd/csrc/semtsdf_steps.h) equals single
additions bit for bit: t, t_prev and the count, stopped by tend, by a count, or by both, and
the sharded march's replay_t composition.  The closed form's count starts from a reciprocal
estimate (the device's rcp); the result must not depend on it, so the checker is also built
with the estimate biased by (1 +- 2^-10), far beyond the device reciprocal's error."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helpers", "march_steps_check.cpp")

ESTIMATES = {
    "exact": [],
    "high": ["-DSEMTSDF_STEPS_RCP(d)=((1.0f+0x1p-10f)/(d))"],
    "low": ["-DSEMTSDF_STEPS_RCP(d)=((1.0f-0x1p-10f)/(d))"],
}


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("estimate", list(ESTIMATES))
def test_skip_steps_equals_single_additions(estimate):
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "chk")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", *ESTIMATES[estimate], "-o", exe, SRC])
        out = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=300)
    res = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in out.stdout.splitlines()}
    cases, bad, closed = res["steps"]
    assert cases >= 1_000_000 and bad == 0, (res, out.stderr)
    assert closed > 0, res  # the closed form (m > 1) was exercised
    assert res["replay"][0] >= 100_000 and res["replay"][1] == 0, (res, out.stderr)
