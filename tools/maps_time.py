#!/usr/bin/env python3
"""Kernel time of the model maps (semtsdf_render_maps_dev) against the label render of the same
views in the same run, on the bench's C3 volume (512^3, semantic, 640 x 480) after --frames
synthetic frames.  Three launches over the bench's orbit views (angle += 0.01 per view at the mean
depth): the label render (semtsdf_raycast_dev, with out_t), the maps with all six outputs, and the
maps with t only.  Times are the library's HIP events around each launch (semtsdf_get_timing:
render_ms / n_render), the three kinds interleaved round by round; per kind the median over the
rounds of the mean time per view, and the rounds' extremes as the run-to-run scatter.  Writes the
result (one JSON line and a readable table, with the build key) to --out."""
import argparse
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
    ap.add_argument("--views", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_maps_time.txt"))
    args = ap.parse_args()

    import semtsdf
    from semtsdf import _lib as L
    from semtsdf.maps import MAP_LAYOUT
    from semtsdf.synth import SyntheticStream

    lib = semtsdf.load()
    st = SyntheticStream(seed=0)
    f0 = st.frame(0)
    mean_m = float(np.mean(f0.depth[f0.depth > 0])) / 5000.0
    p = semtsdf.default_params(args.dim, KI, 640, 480)
    semtsdf.place_from_frame(p, f0.depth, mean_m, L.PLACE_SFM)
    p.flags = L.F_SEMANTIC | L.F_GATE_COLOR
    vol = semtsdf.Volume(p, 0)
    for k in range(1, args.frames + 1):
        fr = st.frame(k)
        vol.integrate(fr.depth, fr.rgb, np.ascontiguousarray(fr.gt_ids), (fr.w2c @ f0.c2w).astype(np.float32))
    vol.sync()

    npx = vol.W * vol.H
    bgr = semtsdf.DeviceBuffer(npx * 3)
    bufs = {k: semtsdf.DeviceBuffer(npx * ch * np.dtype(dt).itemsize) for k, (dt, ch) in MAP_LAYOUT.items()}
    cams = [semtsdf.orbit_camera(list(p.Kinv), 0.01 * (v + 1), mean_m) for v in range(args.views)]
    kinds = {
        "label_render": lambda s2w, c: vol.raycast_dev(s2w, c, L.RENDER_LABEL, bgr.ptr, bufs["t"].ptr),
        "maps_all": lambda s2w, c: vol.render_maps_dev(s2w, c, 1, **{k: b.ptr for k, b in bufs.items()}),
        "maps_t_only": lambda s2w, c: vol.render_maps_dev(s2w, c, 1, t=bufs["t"].ptr),
    }

    def one_round(fn):
        vol.reset_timing()
        for s2w, c in cams:
            fn(s2w, c)
        vol.sync()
        tm = vol.timing()
        assert tm.n_render == len(cams)
        return tm.render_ms / tm.n_render

    for fn in kinds.values():  # warm-up: code objects loaded, the empty-space maps built
        for s2w, c in cams[:4]:
            fn(s2w, c)
    vol.sync()
    vol.set_instrumentation(events=True, count=False)
    ms = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k, fn in kinds.items():
            ms[k].append(one_round(fn))
    vol.set_instrumentation(events=False, count=False)

    flags = np.empty((vol.H, vol.W), np.uint8)
    kinds["maps_all"](*cams[-1])
    bufs["flags"].download(flags, vol.stream)
    vol.sync()
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {
        "tool": "maps_time", "volume": [args.dim] * 3, "frames": args.frames, "views": args.views,
        "rounds": args.rounds, "image": [vol.W, vol.H],
        "ms_per_view": {k: round(med[k], 4) for k in ms},
        "ms_per_view_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
        "maps_all_over_label_render": round(med["maps_all"] / med["label_render"], 3),
        "maps_t_only_over_label_render": round(med["maps_t_only"] / med["label_render"], 3),
        "last_view_hit_share": round(float(((flags & 1) != 0).mean()), 3),
        "last_view_normal_share_of_hits": round(float(((flags & 2) != 0).sum() / max(1, ((flags & 1) != 0).sum())), 3),
        "build_key": lib.semtsdf_build_key().decode()[:16],
    }
    lines = [
        f"model maps, kernel time per view (HIP events), {args.dim}^3 semantic after {args.frames} frames, "
        f"{vol.W} x {vol.H}, {args.views} orbit views x {args.rounds} rounds, kinds interleaved",
        f"build key {res['build_key']}",
        "",
        f"{'launch':<16}{'median ms':>12}{'min ms':>10}{'max ms':>10}{'/ label render':>16}",
    ]
    for k in ms:
        lines.append(f"{k:<16}{med[k]:>12.4f}{min(ms[k]):>10.4f}{max(ms[k]):>10.4f}{med[k] / med['label_render']:>16.3f}")
    lines += [
        "",
        "All three launches run the same march (march_ray) over the same rays.  Beyond it, per hit:",
        "  label_render  the histogram bins present at the hit sampled trilinearly, argmax, palette; stores 3 B BGR + t",
        "  maps_all      the same histogram samples, six more trilinear sdf samples and their 48 weights (normal, flags);",
        "                stores 34 B per pixel",
        "  maps_t_only   nothing; stores t (4 B per pixel)",
        "", json.dumps(res)]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, flush=True)
    for b in [bgr, *bufs.values()]:
        b.free()
    vol.close()


if __name__ == "__main__":
    main()
