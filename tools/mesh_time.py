#!/usr/bin/env python3
"""Time of semtsdf_extract_mesh on the bench's C3 volume (512^3, semantic) after 20 synthetic
frames: wall time around the synchronising call, count-only and full, warm-up then the median
of --runs runs.  Prints one JSON line: milliseconds, vertex and triangle counts, scratch bytes,
and the ratio of the count-only time to the time one read of sdf and weight (8 B per voxel)
takes at the bandwidth semtsdf_copy_bandwidth measures."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-maskrcnn_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

KI = (520.9, 521.0, 325.1, 249.7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import semtsdf
    from semtsdf import _lib as L
    from semtsdf.synth import SyntheticStream

    lib = semtsdf.load()
    st = SyntheticStream(seed=0)
    f0 = st.frame(0)
    p = semtsdf.default_params(args.dim, KI, 640, 480)
    semtsdf.place_from_frame(p, f0.depth, float(np.mean(f0.depth[f0.depth > 0])) / 5000.0, L.PLACE_SFM)
    p.flags = L.F_SEMANTIC | L.F_GATE_COLOR
    vol = semtsdf.Volume(p, 0)
    for k in range(1, args.frames + 1):
        fr = st.frame(k)
        vol.integrate(fr.depth, fr.rgb, np.ascontiguousarray(fr.gt_ids), (fr.w2c @ f0.c2w).astype(np.float32))
    vol.sync()

    nv, nt = C.c_uint64(), C.c_uint64()

    def count_only():
        L.check(lib.semtsdf_extract_mesh(vol.handle, 1, None, 0, None, 0, C.byref(nv), C.byref(nt)))

    count_only()
    n, m = int(nv.value), int(nt.value)
    rec = np.zeros(max(n, 1) * 32, np.uint8)
    faces = np.zeros(max(m, 1) * 3, np.uint32)

    def full():
        L.check(lib.semtsdf_extract_mesh(vol.handle, 1, rec.ctypes.data, n, faces.ctypes.data, m, C.byref(nv),
                                         C.byref(nt)))

    def median_ms(fn):
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.runs):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e3)
        return statistics.median(ts), min(ts)

    count_ms, count_min = median_ms(count_only)
    full_ms, full_min = median_ms(full)
    gbs = C.c_double()
    stored = int(vol.state().local_voxels)
    ny, nz = (args.dim + 7) // 8 * 8, (args.dim + 31) // 32 * 32
    tiled = args.dim * ny * nz  # the tiled storage pads y to 8 rows and z to 32 planes
    L.check(lib.semtsdf_copy_bandwidth(0, 1 << 30, 5, C.byref(gbs)))
    floor_ms = 8.0 * stored / (gbs.value * 1e9) * 1e3
    tiles = tiled // 256
    scratch_count = tiles * 28 + (args.dim + 3) // 4 * (tiles // args.dim) * 4 + (tiles + 4095) // 4096 * 16 + 24
    print(json.dumps({
        "tool": "mesh_time", "volume": [args.dim] * 3, "frames": args.frames, "runs": args.runs,
        "count_only_ms": round(count_ms, 3), "count_only_min_ms": round(count_min, 3),
        "full_ms": round(full_ms, 3), "full_min_ms": round(full_min, 3),
        "vertices": n, "triangles": m,
        "scratch_bytes_count": scratch_count,
        "scratch_bytes_full": scratch_count + tiled * 4 + n * 32 + m * 12,
        "copy_bandwidth_gbs": round(gbs.value, 1), "one_read_floor_ms": round(floor_ms, 3),
        "count_over_floor": round(count_ms / floor_ms, 2),
        "build_key": lib.semtsdf_build_key().decode()[:16],
    }), flush=True)
    vol.close()


if __name__ == "__main__":
    main()
