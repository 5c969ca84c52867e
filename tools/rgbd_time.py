#!/usr/bin/env python3
"""Device time of the RGB-D tracking launches against existing launches on the same inputs in the same
run, and the wall time of one tracked frame with and without the photometric term, on the bench's C3
volume (512^3, semantic, 640 x 480) after --frames synthetic frames.  Four launches, each between two
HIP events (torch.cuda.Event) on one stream: semtsdf_frame_maps_dev (the yardstick of the intensity
pyramid), semtsdf_intensity_pyramid_dev (three levels of the model's colour render with its validity
image), semtsdf_icp_system_level_dev at level 0, stride 1 (the yardstick of the system: the 32-word
kernel, which this tool's subject does not touch) and semtsdf_rgbd_system_level_dev on the same
buffers.  The kinds are interleaved launch by launch; per kind the median over the rounds of the
round's median launch, and the rounds' extremes as the run-to-run scatter.  Then
semtsdf.track.track_pyramid and track_rgbd of the next frame from the constant-pose guess,
alternating, host clock around the whole call.  Writes the result (one JSON line and a readable table,
with the build key) to --out."""
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
GATES = dict(dist_max=0.1, cos_min=0.8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tracks", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgbd_time.txt"))
    args = ap.parse_args()

    import torch

    import semtsdf
    from semtsdf import _lib as L
    from semtsdf.maps import pose_camera
    from semtsdf.synth import SyntheticStream
    from semtsdf.track import R_MAX, pose_errors, rgbd_system_from_words, track_pyramid, track_rgbd

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
    rgb = np.ascontiguousarray(nxt.rgb)
    E_true = (nxt.w2c @ f0.c2w).astype(np.float32)

    npx = vol.W * vol.H
    geo = vol.frame_levels(3)
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    sizes = {"depth": 2 * npx, "rgb": 3 * npx, "m_rgb": 3 * npx, "m_valid": npx, "vertex": 12 * npx, "normal": 12 * npx,
             "flags": npx, "m_point": 12 * npx, "m_normal": 12 * npx, "m_flags": npx, "words": 8 * L.RGBD_WORDS}
    per = {"z": 4, "vertex": 12, "normal": 12, "flags": 1, "fS": 4, "fV": 1, "mS": 4, "mV": 1}
    for l, g in enumerate(geo):
        sizes.update({f"{k}{l}": b * g["width"] * g["height"] for k, b in per.items()})
    bufs = {k: semtsdf.DeviceBuffer(s) for k, s in sizes.items()}
    s2w, cam = pose_camera(list(p.Kinv), E)
    vol.render_maps_dev(s2w, cam, 1, stream=sp, point=bufs["m_point"].ptr, normal=bufs["m_normal"].ptr,
                        flags=bufs["m_flags"].ptr)
    vol.raycast_dev(s2w, cam, L.RENDER_COLOR, bufs["m_rgb"].ptr, stream=sp)
    m_flags = np.zeros(npx, np.uint8)
    bufs["m_flags"].download(m_flags, sp)
    stream.synchronize()
    m_valid = np.ascontiguousarray((m_flags & 3) == 3, dtype=np.uint8)
    bufs["m_valid"].upload(m_valid, sp)
    bufs["depth"].upload(depth, sp)
    bufs["rgb"].upload(rgb, sp)
    vol.frame_pyramid_dev(bufs["depth"].ptr, [{k: bufs[f"{k}{l}"].ptr for k in ("z", "vertex", "normal", "flags")}
                                              for l in range(3)], 3, 0.05, 0.15, stream=sp)
    f_levels = [{"S": bufs[f"fS{l}"].ptr, "valid": bufs[f"fV{l}"].ptr} for l in range(3)]
    m_levels = [{"S": bufs[f"mS{l}"].ptr, "valid": bufs[f"mV{l}"].ptr} for l in range(3)]
    vol.intensity_pyramid_dev(bufs["rgb"].ptr, None, f_levels, stream=sp)
    vol.intensity_pyramid_dev(bufs["m_rgb"].ptr, bufs["m_valid"].ptr, m_levels, stream=sp)
    maps = [bufs[k].ptr for k in ("vertex0", "normal0", "flags0", "m_point", "m_normal", "m_flags")]
    photo = [bufs[k].ptr for k in ("fS0", "fV0", "mS0", "mV0")]
    wp = bufs["words"].ptr
    kinds = {
        "frame_maps": lambda: vol.frame_maps_dev(bufs["depth"].ptr, bufs["vertex"].ptr, bufs["normal"].ptr,
                                                 bufs["flags"].ptr, stream=sp),
        "intensity_pyr": lambda: vol.intensity_pyramid_dev(bufs["m_rgb"].ptr, bufs["m_valid"].ptr, m_levels, stream=sp),
        "icp_system": lambda: vol.icp_system_level_dev(maps, vol.W, vol.H, E, E, GATES["dist_max"], GATES["cos_min"], 1, wp,
                                                       stream=sp),
        "rgbd_system": lambda: vol.rgbd_system_level_dev(maps, photo, 0, E, E, GATES["dist_max"], GATES["cos_min"], R_MAX, 1,
                                                         wp, stream=sp),
    }

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
    words = np.zeros(L.RGBD_WORDS, np.int64)  # of the last launch: the timed system's size
    kinds["rgbd_system"]()
    bufs["words"].download(words, sp)
    stream.synchronize()
    (_, _, _, gc), (_, _, _, pc) = rgbd_system_from_words(words)

    trackers = {"track_pyramid": lambda: track_pyramid(vol, depth, E, E), "track_rgbd": lambda: track_rgbd(vol, depth, rgb, E, E)}
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
            if "photo_inliers" in log[-1]:
                ends[k]["photo_inliers"] = log[-1]["photo_inliers"]
    t_g, r_g = pose_errors(E, E_true)
    wmed = {k: statistics.median(v) for k, v in wall.items()}
    ratios = {"intensity_pyr/frame_maps": round(med["intensity_pyr"] / med["frame_maps"], 3),
              "rgbd_system/icp_system": round(med["rgbd_system"] / med["icp_system"], 3)}
    res = {
        "tool": "rgbd_time", "volume": [args.dim] * 3, "frames": args.frames, "launches": args.launches,
        "rounds": args.rounds, "image": [vol.W, vol.H], "levels": [[g["width"], g["height"]] for g in geo],
        "ms_per_launch": {k: round(med[k], 4) for k in ms},
        "ms_per_launch_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
        "ratios": ratios, "system_counts": {"geometric": gc, "photometric": pc},
        "track_wall_ms": {k: round(wmed[k], 3) for k in wall},
        "track_wall_ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in wall.items()},
        "track_end": ends, "guess": {"t_err_mm": round(t_g * 1e3, 3), "r_err_rad": round(r_g, 5)},
        "build_key": lib.semtsdf_build_key().decode()[:16],
    }
    lines = [
        f"RGB-D tracking, device time per call (HIP events around each call), {vol.W} x {vol.H}, "
        f"{args.launches} launches x {args.rounds} rounds, kinds interleaved",
        f"build key {res['build_key']}",
        "",
        f"{'call':<16}{'median ms':>12}{'min ms':>10}{'max ms':>10}",
    ]
    for k in ms:
        lines.append(f"{k:<16}{med[k]:>12.4f}{min(ms[k]):>10.4f}{max(ms[k]):>10.4f}")
    lines += [
        "",
        f"intensity_pyr / frame_maps = {ratios['intensity_pyr/frame_maps']}    "
        f"rgbd_system / icp_system = {ratios['rgbd_system/icp_system']}",
        "",
        "  frame_maps     semtsdf_frame_maps_dev: one launch, 3 depth loads, 25 B stored per pixel",
        "  intensity_pyr  semtsdf_intensity_pyramid_dev: one launch, three levels of the model's colour render with its",
        "                 validity image, 4 B read per pixel, 5 B stored per level pixel",
        "  icp_system     semtsdf_icp_system_level_dev, level 0 of the radius-3 depth pyramid, stride 1, with its memset",
        "  rgbd_system    semtsdf_rgbd_system_level_dev on the same buffers and both intensity pyramids' level 0, with",
        f"                 its memset; geometric {json.dumps(gc)}, photometric {json.dumps(pc)}",
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
    for b in bufs.values():
        b.free()
    vol.close()


if __name__ == "__main__":
    main()
