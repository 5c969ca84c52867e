#!/usr/bin/env python3
"""Time of semtsdf_shift against the copy bandwidth of the same run, on the bench's C3 volume
(512^3, semantic, 640 x 480) after --frames synthetic frames.  The shifts (8,0,0), (0,8,0), (0,0,8)
and (8,8,-8), --rounds times each, interleaved; per shift the time between two HIP events recorded
around the call on the stream it runs on (its allocations and the launches of all arrays
included; the rebuild of the empty-space maps by the next march is not part of a shift), the bytes
the scheme reads and writes, and the resulting GB/s beside semtsdf_copy_bandwidth.  The same
measurement runs twice, each in a child process of its own: with plain loads and stores
(SEMTSDF_SHIFT_NT=0, read once when the library first shifts) and with the non-temporal ones the
library uses by default.  Writes a readable table and one JSON line, with the build key, to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-maskrcnn_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

KI = (520.9, 521.0, 325.1, 249.7)
SHIFTS = [(8, 0, 0), (0, 8, 0), (0, 0, 8), (8, 8, -8)]


def scheme_bytes(nvox: int, semantic: bool) -> dict:
    """Bytes read plus written per stored voxel array, for narrow storage (u16 weights, u8x4 colour):
    every array is read once and written once into another buffer; a histogram plane is then copied
    back from the spare (a second read and write)."""
    b = {"sdf": 8 * nvox, "weight_u16": 4 * nvox, "colour_u8x4": 8 * nvox}
    if semantic:
        b["bin_mask"] = 8 * nvox
        b["histogram_shift"] = 32 * 8 * nvox
        b["histogram_copy_back"] = 32 * 8 * nvox
    return b


def measure(args) -> dict:
    import torch

    import semtsdf
    from semtsdf import _lib as L
    from semtsdf.synth import SyntheticStream
    import ctypes as C

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
    ny, nz = (args.dim + 7) // 8 * 8, (args.dim + 31) // 32 * 32
    nvox = args.dim * ny * nz  # stored voxels of the tiled layout
    by = scheme_bytes(nvox, True)
    total = sum(by.values())

    gbs = C.c_double(0)
    L.check(lib.semtsdf_copy_bandwidth(0, 1 << 30, 10, C.byref(gbs)))
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)

    def one(shift):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        vol.shift(*shift, stream=sp)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for s in SHIFTS:  # warm-up: code objects loaded
        one(s)
        one(tuple(-c for c in s))
    ms = {s: [] for s in SHIFTS}
    for _ in range(args.rounds):
        for s in SHIFTS:
            ms[s].append(one(s))
            one(tuple(-c for c in s))  # back again: the volume does not walk away over the rounds
    gbs2 = C.c_double(0)
    L.check(lib.semtsdf_copy_bandwidth(0, 1 << 30, 10, C.byref(gbs2)))
    res = {
        "nontemporal": bool(int(os.environ.get("SEMTSDF_SHIFT_NT", "1") or 0)),
        "volume": [args.dim] * 3, "stored_voxels": nvox, "frames": args.frames, "rounds": args.rounds,
        "bytes_per_shift": total, "bytes_by_array": by,
        "ms": {",".join(map(str, s)): round(statistics.median(v), 3) for s, v in ms.items()},
        "ms_min_max": {",".join(map(str, s)): [round(min(v), 3), round(max(v), 3)] for s, v in ms.items()},
        "gbs": {",".join(map(str, s)): round(total / statistics.median(v) / 1e6, 1) for s, v in ms.items()},
        "copy_bandwidth_gbs": [round(gbs.value, 1), round(gbs2.value, 1)],
        "build_key": lib.semtsdf_build_key().decode()[:16],
    }
    vol.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child", action="store_true", help="measure and print one JSON line (used for the NT run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shift_time.txt"))
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(measure(args)), flush=True)
        return
    runs = []
    for nt in ("0", "1"):  # a fresh process each: the switch is read once, and one volume at a time
        env = dict(os.environ, SEMTSDF_SHIFT_NT=nt)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--dim", str(args.dim), "--frames",
                              str(args.frames), "--rounds", str(args.rounds)], env=env, capture_output=True, text=True,
                             timeout=1500)
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
        if out.returncode != 0 or not line:
            sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
            raise SystemExit(f"measurement (SEMTSDF_SHIFT_NT={nt}) failed with status {out.returncode}")
        runs.append(json.loads(line[0][len("RESULT "):]))
    plain = runs[0]
    lines = [
        f"semtsdf_shift, {args.dim}^3 semantic (u16 weights, u8x4 colour) after {args.frames} frames, "
        f"{args.rounds} rounds per shift, shifts interleaved; HIP events around the call",
        f"build key {plain['build_key']}",
        f"stored voxels {plain['stored_voxels']}, bytes read + written per shift {plain['bytes_per_shift']} "
        f"({plain['bytes_per_shift'] / plain['stored_voxels']:.0f} per voxel)",
        "",
    ]
    for r in runs:
        cb = r["copy_bandwidth_gbs"]
        lines.append(f"{'non-temporal' if r['nontemporal'] else 'plain'} loads and stores; semtsdf_copy_bandwidth "
                     f"(1 GiB, best of 10) before {cb[0]} GB/s, after {cb[1]} GB/s")
        lines.append(f"{'shift':<12}{'median ms':>12}{'min ms':>10}{'max ms':>10}{'GB/s':>10}{'/ copy':>9}")
        for s in r["ms"]:
            lines.append(f"{s:<12}{r['ms'][s]:>12.3f}{r['ms_min_max'][s][0]:>10.3f}{r['ms_min_max'][s][1]:>10.3f}"
                         f"{r['gbs'][s]:>10.1f}{r['gbs'][s] / max(cb):>9.2f}")
        lines.append("")
    by = plain["bytes_by_array"]
    lines += ["bytes by array: " + ", ".join(f"{k} {v}" for k, v in by.items()),
              f"The histogram is {(by['histogram_shift'] + by['histogram_copy_back']) / plain['bytes_per_shift']:.0%} of "
              "the traffic, half of that the copy back from the spare: a plane is never moved in place, and the",
              "32 planes are never duplicated whole.  A shift launches 4 + 2 x 32 kernels, allocates twice and frees "
              "twice; the map rebuild happens in the next march and is not timed here.",
              "", json.dumps({"tool": "shift_time", "runs": runs})]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, flush=True)


if __name__ == "__main__":
    main()
