#!/usr/bin/env python3
"""Device time of the tracking launches against the model maps of the same pose in the same run, on
the bench's C3 volume (512^3, semantic, 640 x 480) after --frames synthetic frames.  Three calls, each
between two HIP events (torch.cuda.Event) on one stream: semtsdf_render_maps_dev with all six outputs
at the pose camera of the last fused frame (the yardstick: an existing kernel), semtsdf_frame_maps_dev
of the next frame's depth, and one semtsdf_icp_system_dev launch (with its 256-byte memset) of that
frame against those maps from the constant-pose guess.  The three kinds are interleaved launch by
launch; per kind the median over the rounds of the round's median launch, and the rounds' extremes as
the run-to-run scatter.  Writes the result (one JSON line and a readable table, with the build key)
to --out."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

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
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_time.txt"))
    args = ap.parse_args()

    import torch

    import semtsdf
    from semtsdf import _lib as L
    from semtsdf.maps import MAP_LAYOUT
    from semtsdf.synth import SyntheticStream
    from semtsdf.track import system_from_words

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
    depth = np.ascontiguousarray(st.frame(args.frames + 1).depth)

    npx = vol.W * vol.H
    maps = {k: semtsdf.DeviceBuffer(npx * ch * np.dtype(dt).itemsize) for k, (dt, ch) in MAP_LAYOUT.items()}
    frame = {"depth": semtsdf.DeviceBuffer(2 * npx), "vertex": semtsdf.DeviceBuffer(12 * npx),
             "normal": semtsdf.DeviceBuffer(12 * npx), "flags": semtsdf.DeviceBuffer(npx)}
    words_d = semtsdf.DeviceBuffer(8 * L.ICP_WORDS)
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    frame["depth"].upload(depth, sp)
    s2w, c = semtsdf.pose_camera(list(p.Kinv), E)
    pointers = [frame["vertex"].ptr, frame["normal"].ptr, frame["flags"].ptr, maps["point"].ptr, maps["normal"].ptr,
                maps["flags"].ptr]
    kinds = {
        "maps_all": lambda: vol.render_maps_dev(s2w, c, 1, stream=sp, **{k: b.ptr for k, b in maps.items()}),
        "frame_maps": lambda: vol.frame_maps_dev(frame["depth"].ptr, frame["vertex"].ptr, frame["normal"].ptr,
                                                 frame["flags"].ptr, stream=sp),
        "icp_system": lambda: vol.icp_system_dev(pointers, E, E, 0.1, 0.8, 1, words_d.ptr, stream=sp),
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

    one_round()  # warm-up: code objects loaded, the empty-space maps built
    rounds = [one_round() for _ in range(args.rounds)]
    ms = {k: [r[k] for r in rounds] for k in kinds}
    words = np.zeros(L.ICP_WORDS, np.int64)
    words_d.download(words, sp)
    stream.synchronize()
    counts = system_from_words(words)[3]
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {
        "tool": "icp_time", "volume": [args.dim] * 3, "frames": args.frames, "launches": args.launches,
        "rounds": args.rounds, "image": [vol.W, vol.H],
        "ms_per_launch": {k: round(med[k], 4) for k in ms},
        "ms_per_launch_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
        "frame_maps_over_maps_all": round(med["frame_maps"] / med["maps_all"], 4),
        "icp_system_over_maps_all": round(med["icp_system"] / med["maps_all"], 4),
        "counts": counts,
        "build_key": lib.semtsdf_build_key().decode()[:16],
    }
    lines = [
        f"tracking launches, device time per launch (HIP events around each call), {args.dim}^3 semantic after "
        f"{args.frames} frames, {vol.W} x {vol.H}, {args.launches} launches x {args.rounds} rounds, kinds interleaved",
        f"build key {res['build_key']}",
        "",
        f"{'launch':<14}{'median ms':>12}{'min ms':>10}{'max ms':>10}{'/ maps_all':>12}",
    ]
    for k in ms:
        lines.append(f"{k:<14}{med[k]:>12.4f}{min(ms[k]):>10.4f}{max(ms[k]):>10.4f}{med[k] / med['maps_all']:>12.4f}")
    lines += [
        "",
        "  maps_all     semtsdf_render_maps_dev, six outputs, pose camera of the last fused frame (marches the volume)",
        "  frame_maps   semtsdf_frame_maps_dev of the next frame's depth: 3 depth loads, 25 B stored per pixel",
        "  icp_system   semtsdf_icp_system_dev, stride 1, E_cur = E_ref: a 256-B memset, then one launch reading about",
        "               50 B per pixel; classes of the timed launch: " + json.dumps(counts),
        "", json.dumps(res)]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, flush=True)
    for b in [*maps.values(), *frame.values(), words_d]:
        b.free()
    vol.close()


if __name__ == "__main__":
    main()
