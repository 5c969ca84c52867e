#!/usr/bin/env python3
"""Device time of the depth pyramid against the frame maps of the same depth image in the same run,
and the wall time of one tracked frame with and without the pyramid, on the bench's C3 volume (512^3,
semantic, 640 x 480) after --frames synthetic frames.  Four launches, each between two HIP events
(torch.cuda.Event) on one stream: semtsdf_frame_maps_dev (the yardstick: an existing kernel) and
semtsdf_frame_pyramid_dev with three levels and all outputs at radius 0, 3 and 4 (the filter, two
halvings, three maps launches).  The kinds are interleaved launch by launch; per kind the median over
the rounds of the round's median launch, and the rounds' extremes as the run-to-run scatter.  Then
semtsdf.track.track and track_pyramid of the next frame from the constant-pose guess (the last fused
frame's extrinsic, which both converge from), alternating, host clock around the whole call
(allocations, the model maps, the read-back per iteration, the host solve).  Writes the result (one
JSON line and a readable table, with the build key) to --out."""
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
RADII = (0, 3, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tracks", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid_time.txt"))
    args = ap.parse_args()

    import torch

    import semtsdf
    from semtsdf import _lib as L
    from semtsdf.synth import SyntheticStream
    from semtsdf.track import pose_errors, track, track_pyramid

    lib = semtsdf.load()
    st = SyntheticStream(seed=0)
    f0 = st.frame(0)
    mean_m = float(np.mean(f0.depth[f0.depth > 0])) / 5000.0
    p = semtsdf.default_params(args.dim, KI, 640, 480)
    semtsdf.place_from_frame(p, f0.depth, mean_m, L.PLACE_SFM)
    p.flags = L.F_SEMANTIC | L.F_GATE_COLOR
    vol = semtsdf.Volume(p, 0)
    E = None
    for k in range(1, args.frames + 1):
        fr = st.frame(k)
        E = (fr.w2c @ f0.c2w).astype(np.float32)
        vol.integrate(fr.depth, fr.rgb, np.ascontiguousarray(fr.gt_ids), E)
    vol.sync()
    nxt = st.frame(args.frames + 1)
    depth = np.ascontiguousarray(nxt.depth)
    E_true = (nxt.w2c @ f0.c2w).astype(np.float32)

    npx = vol.W * vol.H
    geo = vol.frame_levels(3)
    frame = {"depth": semtsdf.DeviceBuffer(2 * npx), "vertex": semtsdf.DeviceBuffer(12 * npx),
             "normal": semtsdf.DeviceBuffer(12 * npx), "flags": semtsdf.DeviceBuffer(npx)}
    per = {"z": 4, "vertex": 12, "normal": 12, "flags": 1}
    lbufs = [{k: semtsdf.DeviceBuffer(b * g["width"] * g["height"]) for k, b in per.items()} for g in geo]
    levels = [{k: b.ptr for k, b in lv.items()} for lv in lbufs]
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    frame["depth"].upload(depth, sp)
    kinds = {"frame_maps": lambda: vol.frame_maps_dev(frame["depth"].ptr, frame["vertex"].ptr, frame["normal"].ptr,
                                                      frame["flags"].ptr, stream=sp)}
    for r in RADII:
        kinds[f"pyramid_r{r}"] = lambda r=r: vol.frame_pyramid_dev(frame["depth"].ptr, levels, r, 0.05, 0.15, stream=sp)

    def one_round():
        evs = {k: [] for k in kinds}
        for _ in range(args.launches):
            for k, fn in kinds.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn()
                b.record(stream)
                evs[k].append((a, b))
        stream.synchronize()
        return {k: statistics.median(a.elapsed_time(b) for a, b in v) for k, v in evs.items()}

    one_round()  # warm-up: code objects loaded
    rounds = [one_round() for _ in range(args.rounds)]
    ms = {k: [r[k] for r in rounds] for k in kinds}
    med = {k: statistics.median(v) for k, v in ms.items()}

    trackers = {"track": lambda: track(vol, depth, E, E), "track_pyramid": lambda: track_pyramid(vol, depth, E, E)}
    wall = {k: [] for k in trackers}
    ends = {}
    for i in range(args.tracks + 1):  # the first pass is the warm-up
        for k, fn in trackers.items():
            vol.sync()
            t0 = time.perf_counter()
            Ek, log = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if i:
                wall[k].append(dt)
            t_err, r_err = pose_errors(Ek, E_true)
            ends[k] = {"iterations": len(log), "level0_iterations": sum(1 for e in log if e.get("level", 0) == 0),
                       "inliers": log[-1]["inliers"], "t_err_mm": round(t_err * 1e3, 3), "r_err_rad": round(r_err, 5)}
    t_g, r_g = pose_errors(E, E_true)
    wmed = {k: statistics.median(v) for k, v in wall.items()}
    res = {
        "tool": "pyramid_time", "volume": [args.dim] * 3, "frames": args.frames, "launches": args.launches,
        "rounds": args.rounds, "image": [vol.W, vol.H], "levels": [[g["width"], g["height"]] for g in geo],
        "ms_per_launch": {k: round(med[k], 4) for k in ms},
        "ms_per_launch_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
        "over_frame_maps": {k: round(med[k] / med["frame_maps"], 3) for k in ms},
        "track_wall_ms": {k: round(wmed[k], 3) for k in wall},
        "track_wall_ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in wall.items()},
        "track_end": ends, "guess": {"t_err_mm": round(t_g * 1e3, 3), "r_err_rad": round(r_g, 5)},
        "build_key": lib.semtsdf_build_key().decode()[:16],
    }
    lines = [
        f"depth pyramid, device time per call (HIP events around each call), {vol.W} x {vol.H}, 3 levels, "
        f"{args.launches} launches x {args.rounds} rounds, kinds interleaved",
        f"build key {res['build_key']}",
        "",
        f"{'call':<14}{'median ms':>12}{'min ms':>10}{'max ms':>10}{'/ frame_maps':>14}",
    ]
    for k in ms:
        lines.append(f"{k:<14}{med[k]:>12.4f}{min(ms[k]):>10.4f}{max(ms[k]):>10.4f}{med[k] / med['frame_maps']:>14.3f}")
    lines += [
        "",
        "  frame_maps    semtsdf_frame_maps_dev: one launch, 3 depth loads, 25 B stored per pixel",
        "  pyramid_rR    semtsdf_frame_pyramid_dev, radius R, sigma_r 0.05, band 0.15, z and the three maps of all",
        "                three levels: 6 launches (filter, 2 halvings, 3 maps), 29 B stored per level pixel",
        "",
        f"one tracked frame, host clock around the call, {args.dim}^3 semantic after {args.frames} frames, from the "
        f"constant-pose guess ({res['guess']['t_err_mm']} mm, {res['guess']['r_err_rad']} rad off), {args.tracks} calls "
        "each, alternating",
        f"{'call':<16}{'median ms':>12}{'min ms':>10}{'max ms':>10}  end",
    ]
    for k in wall:
        lines.append(f"{k:<16}{wmed[k]:>12.3f}{min(wall[k]):>10.3f}{max(wall[k]):>10.3f}  {json.dumps(ends[k])}")
    lines += ["", json.dumps(res)]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, flush=True)
    for b in [*frame.values(), *[b for lv in lbufs for b in lv.values()]]:
        b.free()
    vol.close()


if __name__ == "__main__":
    main()
