"""bench.py's command line: a plain run prints the headline line alone, --dump-outputs writes the
state the last timed step left, --full adds the other records.

CPU: the sample dump_outputs takes is fixed by its arguments and stays under the 64 MB bound at the
benchmark's 512^3 volume.  GPU: one plain run of the benchmark as a process on a 64^3 volume; its
line and the arrays it wrote against the same steps run here through the ABI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeVolume:
    """download_slab of a volume whose voxel v = (x, y, z) holds values that name it."""

    def __init__(self, dims, flags=0x1):
        self.local_dim = dims

        class P:
            pass

        self.params = P()
        self.params.flags = flags
        self.asked = []

    def download_slab(self, x0, x1, hist=False):
        assert x1 == x0 + 1 and 0 <= x0 < self.local_dim[0]
        self.asked.append(x0)
        n = self.local_dim[1] * self.local_dim[2]
        got = {"sdf": np.zeros(n, np.float32), "wt": np.zeros(n, np.int32), "color": np.zeros(n * 3, np.uint8)}
        got["sdf"][:] = x0
        got["wt"][:] = np.arange(n) % 1000
        got["color"][:] = np.arange(n * 3) % 251
        if hist:
            got["hist"] = np.zeros(n * 32, np.uint32)
            got["hist"][::32] = np.arange(n) % 4093
        return got


def load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.parametrize("dims", [(512, 512, 512), (40, 24, 16), (5, 8, 8)])
def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, dims):
    import bench

    recs, dumps = [], []
    for run in ("a", "b"):
        vol = FakeVolume(dims)
        recs.append(bench.dump_outputs(vol, str(tmp_path / run)))
        dumps.append(load_dir(str(tmp_path / run)))
        assert vol.asked == recs[-1]["x_planes"] == sorted(set(vol.asked))  # distinct planes, each read once
    a, b = dumps
    assert sorted(a) == ["color", "hist", "sdf", "wt"]
    assert all(v.dtype == np.float32 for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)
    total = sum(v.nbytes for v in a.values())
    assert total == recs[0]["bytes"] <= 64_000_000
    plane = dims[1] * dims[2]
    xs = recs[0]["x_planes"]
    assert a["sdf"].shape == a["wt"].shape == (len(xs), plane) and a["color"].shape == (len(xs), plane, 3)
    assert a["hist"].shape == (len(xs), recs[0]["hist_voxels_per_plane"], 32)
    assert np.array_equal(a["sdf"][:, 0], np.array(xs, np.float32))
    assert np.array_equal(a["wt"][0], (np.arange(plane) % 1000).astype(np.float32))
    assert np.array_equal(a["color"][0].reshape(-1), (np.arange(plane * 3) % 251).astype(np.float32))
    # the histogram rows are voxels of the plane, increasing and distinct, and differ from plane to plane
    picked = a["hist"][:, :, 0]
    if plane <= 4093:
        assert (np.diff(picked, axis=1) > 0).all()
    if recs[0]["hist_voxels_per_plane"] < plane and len(xs) > 1:
        assert not np.array_equal(picked[0], picked[1])
    # a volume without histogram writes none
    rec = bench.dump_outputs(FakeVolume(dims, flags=0), str(tmp_path / "c"))
    assert sorted(load_dir(str(tmp_path / "c"))) == ["color", "sdf", "wt"] and rec["hist_voxels_per_plane"] == 0


def test_full_and_dump_outputs_are_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--full" in out.stdout and "--dump-outputs DIR" in out.stdout
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True,
                         text=True, timeout=120)
    assert bad.returncode == 2 and "--steps" in bad.stderr


@pytest.mark.gpu
def test_plain_run_line_and_dumped_state(tmp_path):
    """A plain run at 64^3, 3 timed steps after 2 warm-up steps over 4 frames: the line holds the
    headline fields and none of --full's records; the arrays are the volume state after the same 5
    frames integrated here (semtsdf_integrate_dev_async, as the timed step), plane by plane."""
    import bench
    import semtsdf
    from semtsdf import _lib as L
    from semtsdf.synth import SyntheticStream

    D, steps, warmup, F = 64, 3, 2, 4
    d = str(tmp_path / "out")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                          "--warmup", str(warmup), "--dim", str(D), "--frames", str(F), "--dump-outputs", d],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["metric"] == bench.METRIC and rec["unit"] == "Mvoxel-updates/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "f32" and rec["steps"] == steps and rec["warmup"] == warmup and rec["full"] is False
    assert rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(D ** 3 * 1e3 / rec["ms_per_step"] / 1e6, rel=0.05)  # ms rounded to 1e-4
    for k in ("roofline", "cpu_baseline", "pipeline", "orbit", "mask_producer", "c2", "c4_single_gpu"):
        assert k not in rec
    got = load_dir(d)
    assert sorted(got) == ["color", "hist", "sdf", "wt"] and all(v.dtype == np.float32 for v in got.values())
    assert sum(v.nbytes for v in got.values()) == rec["dump_outputs"]["bytes"] <= 64_000_000

    semtsdf.load()
    st = SyntheticStream(seed=1, noise=True)
    f0 = st.frame(0)
    frames = [st.frame(k) for k in range(1, F + 1)]
    p = bench.place(semtsdf, L, D, f0)
    p.flags = L.F_SEMANTIC | L.F_GATE_COLOR
    vol = semtsdf.Volume(p, 0)
    dbuf, rbuf, mbuf = bench.resident_frames(frames, ids=True)
    for k in range(warmup + steps):
        i = k % F
        E = (frames[i].w2c @ f0.c2w).astype(np.float32)
        vol.integrate_dev_async(dbuf.ptr + i * bench.NPX * 2, rbuf.ptr + i * bench.NPX * 3, mbuf.ptr + i * bench.NPX, E)
    vol.sync()
    xs = rec["dump_outputs"]["x_planes"]
    assert len(xs) == got["sdf"].shape[0] > 1
    touched = 0
    for j, x in enumerate(xs):
        ref = vol.download_slab(x, x + 1, hist=True)
        assert np.array_equal(got["sdf"][j], ref["sdf"]), x
        assert np.array_equal(got["wt"][j], ref["wt"].astype(np.float32)), x
        assert np.array_equal(got["color"][j].reshape(-1), ref["color"].astype(np.float32)), x
        touched += int((ref["wt"] > 0).sum())
    assert touched > 0  # the sampled planes cross the integrated band
    here = str(tmp_path / "here")
    bench.dump_outputs(vol, here)
    assert np.array_equal(load_dir(here)["hist"], got["hist"])
    assert got["hist"].sum() > 0
    for b in (dbuf, rbuf, mbuf):
        b.free()
    vol.close()
