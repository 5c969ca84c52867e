#!/usr/bin/env python3
"""Times of semtsdf_instance_stats and semtsdf_remap_instances on the bench's C3 volume (512^3,
semantic) after 20 synthetic frames: wall time around the synchronised call, warm-up then the
median of --runs runs.  Prints one JSON line: the stats call with and without the overlap table,
one remap merging two populated ids, and two yardsticks measured in the same run -- the
count-only semtsdf_export_surface call (the same selection by the existing kernel) and the time
one read of sdf and weight (8 B per stored voxel; for the remap one read of the bin mask, 4 B)
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

    rec = np.zeros(32 * 96, np.uint8)
    ov = np.zeros(32 * 32, np.uint64)
    n = C.c_uint64()

    def stats_overlap():
        L.check(lib.semtsdf_instance_stats(vol.handle, 0.2, 1, L.ptr(rec), L.ptr(ov)))

    def stats_bare():
        L.check(lib.semtsdf_instance_stats(vol.handle, 0.2, 1, L.ptr(rec), None))

    def surface_count():
        L.check(lib.semtsdf_export_surface(vol.handle, 0.2, 1, None, 0, C.byref(n)))

    info = vol.instance_stats()
    a, b = sorted(int(k) for k in np.argsort(info["voxels"][1:])[-2:] + 1)
    luts = [np.arange(32, dtype=np.uint8), np.arange(32, dtype=np.uint8)]
    luts[0][b] = a  # merge b into a, timed once (a second merge finds bin b empty); the repeated runs swap a and b
    luts[1][[a, b]] = [b, a]
    calls = [0]

    def remap():
        t = luts[0] if calls[0] == 0 else luts[1]
        calls[0] += 1
        L.check(lib.semtsdf_remap_instances(vol.handle, L.ptr(t), -1, None))
        vol.sync()

    def median_ms(fn, warmup=args.warmup):
        for _ in range(warmup):
            fn()
        ts = []
        for _ in range(args.runs):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e3)
        return statistics.median(ts), min(ts)

    ov_ms, ov_min = median_ms(stats_overlap)
    bare_ms, bare_min = median_ms(stats_bare)
    surf_ms, surf_min = median_ms(surface_count)
    moved = int(info["support"][b])
    # the first call merges b into a (the voxels with bin b move); every later one swaps a and b,
    # which moves the voxels with bin a: the merged support
    t0 = time.perf_counter()
    remap()
    merge_ms = (time.perf_counter() - t0) * 1e3
    swap_ms, swap_min = median_ms(remap)
    gbs = C.c_double()
    ny, nz = (args.dim + 7) // 8 * 8, (args.dim + 31) // 32 * 32
    tiled = args.dim * ny * nz  # the tiled storage pads y to 8 rows and z to 32 planes
    L.check(lib.semtsdf_copy_bandwidth(0, 1 << 30, 5, C.byref(gbs)))
    floor8 = 8.0 * tiled / (gbs.value * 1e9) * 1e3
    floor4 = 4.0 * tiled / (gbs.value * 1e9) * 1e3
    print(json.dumps({
        "tool": "instance_time", "volume": [args.dim] * 3, "frames": args.frames, "runs": args.runs,
        "selected_voxels": int(info["voxels"].sum()), "populated_ids": int((info["voxels"][1:] > 0).sum()),
        "stats_overlap_ms": round(ov_ms, 3), "stats_overlap_min_ms": round(ov_min, 3),
        "stats_ms": round(bare_ms, 3), "stats_min_ms": round(bare_min, 3),
        "export_surface_count_ms": round(surf_ms, 3), "export_surface_count_min_ms": round(surf_min, 3),
        "remap_merge_first_ms": round(merge_ms, 3), "remap_merge_moved_support": moved,
        "remap_swap_ms": round(swap_ms, 3), "remap_swap_min_ms": round(swap_min, 3),
        "copy_bandwidth_gbs": round(gbs.value, 1),
        "one_read_sdf_wt_ms": round(floor8, 3), "one_read_hmask_ms": round(floor4, 3),
        "stats_over_floor": round(bare_ms / floor8, 2), "stats_overlap_over_floor": round(ov_ms / floor8, 2),
        "remap_over_floor": round(swap_ms / floor4, 2),
        "build_key": lib.semtsdf_build_key().decode()[:16],
    }), flush=True)
    vol.close()


if __name__ == "__main__":
    main()
