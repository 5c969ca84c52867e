#!/usr/bin/env python3
"""Time and size of the brick paging calls on the bench's C3 volume (512^3, semantic, 640 x 480)
after --frames synthetic frames.  For a one-brick-thick face slab on each axis, as a shift of 8 voxels
pushes out (of the two faces the one with more occupied bricks, named by its brick index), and for the
whole volume: the occupied bricks, the packed bytes against the dense bytes of the
box (44 B per voxel of narrow storage plus the bin mask: sdf 4, weight 2, colour 4, mask 4,
histogram 128 -- what a dense download of the box would move, 142 B), and per call the median over
--rounds of
  count   HIP events around the count-only semtsdf_pack_bricks: occupancy and scan kernels, 16 B back
  pack    HIP events around, and host wall time of, the filling semtsdf_pack_bricks (the count pass
          again, the gather, the copies into pageable host memory)
  unpack  the same two for semtsdf_unpack_bricks of those records into the same volume
The events are recorded on the handle's own stream, which both calls use and drain, so an event
time is the device-side span of the call, host gaps between its launches included.  Beside them
semtsdf_copy_bandwidth from the same run, and the paged follow itself: semtsdf.bricks.shift_paged
into a BrickStore by (8, 0, 0), (0, 0, 8) and (8, 8, -8) and back again, host wall time of each leg
(the packs, BrickStore.put, the shift, BrickStore.take, the unpacks; the way out stores what leaves,
the way back returns it), against the wall time of the plain Volume.shift by the same vector,
measured afterwards because a plain shift loses what leaves.  Writes a readable table and one JSON
line, with the build key, to --out."""
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
DENSE_BYTES_PER_VOXEL = 4 + 2 + 4 + 4 + 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bricks_time.txt"))
    args = ap.parse_args()

    import torch

    import semtsdf
    from semtsdf import _lib as L
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
    gbs = C.c_double(0)
    L.check(lib.semtsdf_copy_bandwidth(0, 1 << 30, 10, C.byref(gbs)))
    stream = torch.cuda.ExternalStream(vol.stream)
    nb = vol.brick_counts()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        t0 = time.perf_counter()
        out = fn()
        wall = (time.perf_counter() - t0) * 1e3
        e1.record(stream)
        e1.synchronize()
        return out, e0.elapsed_time(e1), wall

    def count_only(lo, hi):
        lo, hi = np.array(lo, np.int32), np.array(hi, np.int32)
        n, m = C.c_uint64(0), C.c_uint64(0)
        L.check(lib.semtsdf_pack_bricks(vol.handle, L.ptr(lo), L.ptr(hi), None, 0, None, 0, C.byref(n), C.byref(m)))
        return n.value, m.value

    boxes = {}
    for a, axis in enumerate("xyz"):  # of the two face slabs of an axis, the one that holds more
        faces = []
        for b in (0, nb[a] - 1):
            lo, hi = [0, 0, 0], list(nb)
            lo[a], hi[a] = b, b + 1
            faces.append((count_only(lo, hi)[0], f"{axis}-slab {b}", (tuple(lo), tuple(hi))))
        _, name, box = max(faces, key=lambda f: f[0])
        boxes[name] = box
    boxes["whole"] = ((0, 0, 0), nb)
    rows = {}
    for name, (lo, hi) in boxes.items():
        rounds = 1 if name == "whole" else args.rounds
        count_only(lo, hi)  # warm-up: code objects loaded
        cnt, pk, up = [], [], []
        for _ in range(rounds):
            (nbr, nw), ev, _ = timed(lambda: count_only(lo, hi))
            cnt.append(ev)
            (bricks, words), ev, wall = timed(lambda: vol.pack_bricks(lo, hi))
            pk.append((ev, wall))
            _, ev, wall = timed(lambda: vol.unpack_bricks(bricks, words))
            up.append((ev, wall))
        box_voxels = 512 * int(np.prod([h - l for l, h in zip(lo, hi)]))
        med = statistics.median
        rows[name] = {"box_bricks": box_voxels // 512, "occupied": int(nbr), "packed_bytes": int(nw) * 4 + int(nbr) * 24,
                      "dense_bytes": box_voxels * DENSE_BYTES_PER_VOXEL, "rounds": rounds,
                      "count_event_ms": round(med(cnt), 3),
                      "pack_event_ms": round(med(e for e, _ in pk), 3), "pack_wall_ms": round(med(w for _, w in pk), 3),
                      "unpack_event_ms": round(med(e for e, _ in up), 3),
                      "unpack_wall_ms": round(med(w for _, w in up), 3)}
        del bricks, words
    from semtsdf.bricks import BrickStore, shift_paged

    def wall_ms(fn):
        vol.sync()
        t0 = time.perf_counter()
        fn()
        vol.sync()
        return (time.perf_counter() - t0) * 1e3

    med = statistics.median
    walks = {"8,0,0": (8, 0, 0), "0,0,8": (0, 0, 8), "8,8,-8": (8, 8, -8)}
    paged = {}
    for name, s in walks.items():
        back = tuple(-c for c in s)
        store = BrickStore()
        out_ms, back_ms, kept = [], [], (0, 0)
        for _ in range(args.rounds + 1):  # the first round loads what is not loaded yet
            out_ms.append(wall_ms(lambda: shift_paged(vol, store, s)))
            kept = (len(store), store.nbytes)
            back_ms.append(wall_ms(lambda: shift_paged(vol, store, back)))
            assert len(store) == 0 and store.origin == [0, 0, 0]
        paged[name] = {"stored_bricks": kept[0], "stored_bytes": kept[1], "out_ms": round(med(out_ms[1:]), 3),
                       "back_ms": round(med(back_ms[1:]), 3)}
    sh = []
    for name, s in walks.items():  # last: these lose what leaves
        ms = []
        for _ in range(args.rounds + 1):
            ms.append(wall_ms(lambda: vol.shift(*s)))
            vol.shift(*(-c for c in s))
        paged[name]["plain_ms"] = round(med(ms[1:]), 3)
        if name == "8,0,0":
            for _ in range(args.rounds):
                _, ev, _ = timed(lambda: vol.shift(*s))
                sh.append(ev)
                vol.shift(*(-c for c in s))
    gbs2 = C.c_double(0)
    L.check(lib.semtsdf_copy_bandwidth(0, 1 << 30, 10, C.byref(gbs2)))
    shift_ms = statistics.median(sh)
    res = {"tool": "bricks_time", "volume": [args.dim] * 3, "frames": args.frames, "boxes": rows, "paged_follow": paged,
           "shift_ms": round(shift_ms, 3), "copy_bandwidth_gbs": [round(gbs.value, 1), round(gbs2.value, 1)],
           "build_key": lib.semtsdf_build_key().decode()[:16]}
    lines = [f"semtsdf_pack_bricks / semtsdf_unpack_bricks, {args.dim}^3 semantic (u16 weights, u8x4 colour) after "
             f"{args.frames} frames; medians of {args.rounds} rounds (whole volume: 1)",
             f"build key {res['build_key']}",
             f"semtsdf_copy_bandwidth (1 GiB, best of 10) before {res['copy_bandwidth_gbs'][0]} GB/s, after "
             f"{res['copy_bandwidth_gbs'][1]} GB/s; semtsdf_shift by 8 voxels in x: {shift_ms:.3f} ms (HIP events)",
             "",
             f"{'box':<12}{'bricks':>8}{'occupied':>10}{'packed MB':>11}{'dense MB':>10}{'ratio':>8}{'count ms':>10}"
             f"{'pack ev':>10}{'pack wall':>11}{'unpack ev':>11}{'unp. wall':>11}"]
    for name, r in rows.items():
        lines.append(f"{name:<12}{r['box_bricks']:>8}{r['occupied']:>10}{r['packed_bytes'] / 1e6:>11.2f}"
                     f"{r['dense_bytes'] / 1e6:>10.1f}{r['packed_bytes'] / r['dense_bytes']:>8.4f}{r['count_event_ms']:>10.3f}"
                     f"{r['pack_event_ms']:>10.3f}{r['pack_wall_ms']:>11.3f}{r['unpack_event_ms']:>11.3f}"
                     f"{r['unpack_wall_ms']:>11.3f}")
    lines.append("")
    lines.append("paged follow (semtsdf.bricks.shift_paged into a BrickStore, host wall time of the whole leg) against the "
                 "plain Volume.shift by the same vector")
    lines.append(f"{'shift':<10}{'stored':>8}{'MB':>8}{'out ms':>10}{'back ms':>10}{'plain ms':>10}{'out/plain':>11}"
                 f"{'back/plain':>12}")
    for name, r in paged.items():
        lines.append(f"{name:<10}{r['stored_bricks']:>8}{r['stored_bytes'] / 1e6:>8.2f}{r['out_ms']:>10.3f}{r['back_ms']:>10.3f}"
                     f"{r['plain_ms']:>10.3f}{r['out_ms'] / r['plain_ms']:>11.3f}{r['back_ms'] / r['plain_ms']:>12.3f}")
    lines += ["", json.dumps(res)]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, flush=True)
    vol.close()


if __name__ == "__main__":
    main()
