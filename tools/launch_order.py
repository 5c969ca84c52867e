#!/usr/bin/env python3
"""Launch order of the host API, per build, for changes to semtsdf_api.cpp that must not move a kernel
launch or a copy.

  drive    the program to trace: two frames through every host-pointer entry point and every _dev
           twin on the handle's own stream, one filter_overlaps_dev, one sharded association apply
           that decides from the reduced sums and one that needs the pixels (NEED_PIXELS, then
           apply_exact).  64^3, 75 x 53.  The library is the one SEMTSDF_LIB names.
               rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d DIR -o run -- \
                   python3 tools/launch_order.py drive
  compare  DIR_A DIR_B [OUT]: per stream, the ordered kernel names and copy directions of the two
           traces (run-length encoded) and whether they are equal; streams are matched by content.
           A trace without a stream column is compared by the counts per name.  Exit status 1 when
           the builds differ.
"""
import collections
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, KI = 75, 53, (61.0, 61.1, 38.1, 27.6)


def drive():
    sys.path.insert(0, os.path.join(ROOT, "slam-maskrcnn_amd"))
    import numpy as np
    import semtsdf
    from semtsdf import _lib as L
    from semtsdf.shard import LocalShardGroup
    from semtsdf.synth import SyntheticStream
    from semtsdf.volume import DeviceBuffer

    semtsdf.load()
    st = SyntheticStream(seed=0, width=W, height=H, intrinsics=KI, min_area=25)
    fr = [st.frame(k) for k in range(9)]
    Es = [(f.w2c @ fr[0].c2w).astype(np.float32) for f in fr]
    n = W * H

    def params(shard=None):
        p = semtsdf.default_params(64, KI, W, H)
        semtsdf.place_from_frame(p, fr[0].depth, float(np.mean(fr[0].depth[fr[0].depth > 0])) / 5000.0, L.PLACE_SFM)
        p.flags = L.F_SEMANTIC | L.F_GATE_COLOR
        if shard is not None:
            p.z_nshards, p.z_shard, p.z_chunk = 2, shard, 16
        return p

    p = params()
    s2w, c = semtsdf.orbit_camera(list(p.Kinv), 0.2, p.vol_start[2] + 0.5 * (p.vol_end[2] - p.vol_start[2]))

    # ---- the host-pointer entry points
    a = semtsdf.Volume(p, 0)
    for k in (1, 2):
        a.parse_frame(fr[k].depth, fr[k].rgb, fr[k].mask.copy(), Es[k])
    for k in (3, 4):
        m = fr[k].mask.copy()
        a.associate(m, Es[k])
        a.integrate(fr[k].depth, fr[k].rgb, m, Es[k])
    for k in (5, 6):
        probs, box = a.assoc_probs(Es[k])
        a.raycast(s2w, c, L.RENDER_LABEL, want_t=True)
        model = a.render_maps(s2w, c, 1)
        frame = a.frame_maps(fr[k].depth)
        a.icp_system(frame, model, Es[k], Es[k])

    # ---- their _dev twins, on the handle's own stream
    b = semtsdf.Volume(p, 0)
    d_b, r_b, m_b = DeviceBuffer(n * 2), DeviceBuffer(n * 3), DeviceBuffer(n)
    img, t_b = DeviceBuffer(n * 3), DeviceBuffer(n * 4)
    maps = {"t": DeviceBuffer(n * 4), "point": DeviceBuffer(n * 12), "normal": DeviceBuffer(n * 12),
            "label": DeviceBuffer(n), "votes": DeviceBuffer(n * 4), "flags": DeviceBuffer(n)}
    vtx, nrm, flg, words = DeviceBuffer(n * 12), DeviceBuffer(n * 12), DeviceBuffer(n), DeviceBuffer(8 * L.ICP_WORDS)

    def upload(k):
        d_b.upload(fr[k].depth, b.stream)
        r_b.upload(fr[k].rgb, b.stream)
        m_b.upload(fr[k].mask, b.stream)

    for k in (1, 2):
        upload(k)
        b.parse_frame_dev(d_b.ptr, r_b.ptr, m_b.ptr, Es[k])
    for k in (3, 4):
        upload(k)
        b.associate_dev(m_b.ptr, Es[k], want_stats=(k == 3))
        b.integrate_dev(d_b.ptr, r_b.ptr, m_b.ptr, Es[k])
    for k in (5, 6):
        upload(k)
        b.associate_dev(m_b.ptr, Es[k])
        b.integrate_dev_async(d_b.ptr, r_b.ptr, m_b.ptr, Es[k])
    for k in (7, 8):
        upload(k)
        b.parse_frame_view_dev(d_b.ptr, r_b.ptr, m_b.ptr, Es[k], s2w, c, L.RENDER_LABEL, img.ptr)
    for k in (7, 8):
        b.raycast_dev(s2w, c, L.RENDER_LABEL, img.ptr, t_b.ptr)
        b.render_maps_dev(s2w, c, 1, **{name: buf.ptr for name, buf in maps.items()})
        b.frame_maps_dev(d_b.ptr, vtx.ptr, nrm.ptr, flg.ptr)
        b.icp_system_dev((vtx.ptr, nrm.ptr, flg.ptr, maps["point"].ptr, maps["normal"].ptr, maps["flags"].ptr),
                         Es[k], Es[k], 0.1, 0.8, 1, words.ptr)
    b.sync()
    pr_b, bx_b = DeviceBuffer(probs.nbytes), DeviceBuffer(box.nbytes)
    pr_b.upload(probs, b.stream)
    bx_b.upload(box, b.stream)
    m_b.upload(fr[8].mask, b.stream)
    b.filter_overlaps_dev(pr_b.ptr, bx_b.ptr, m_b.ptr)
    b.sync()

    # ---- the sharded association: decided from the reduced sums, then needing the pixels
    shards = [semtsdf.Volume(params(s), 0) for s in range(2)]
    grp = LocalShardGroup(shards, exchange="allgather")
    masks = [DeviceBuffer(n) for _ in shards]

    def shard_frame(k):
        d_b.upload(fr[k].depth, grp.stream)
        r_b.upload(fr[k].rgb, grp.stream)
        for mb in masks:
            mb.upload(fr[k].mask, grp.stream)
        if k > 1:
            grp.associate_dev([mb.ptr for mb in masks], Es[k], want_stats=True)
        for v, mb in zip(shards, masks):
            v.integrate_dev(d_b.ptr, r_b.ptr, mb.ptr, Es[k], grp.stream)

    shard_frame(1)
    shard_frame(2)
    for v in shards:
        v.set_instrumentation(events=False, force_exact=True)
    shard_frame(3)
    shards[0].sync()
    for v in (a, b, *shards):
        v.close()
    print("launch_order: drive done")


def short(name):
    head = name.split("(")[0].strip() or name  # without the argument list
    return head[5:] if head.startswith("void ") else head


def read_trace(d):
    """{stream or None: {"kernels": [names in start order], "copies": [directions in start order]}}"""
    rows = []
    for pat, col, kind in (("*kernel_trace.csv", "Kernel_Name", "kernels"),
                           ("*memory_copy_trace.csv", "Direction", "copies")):
        files = glob.glob(os.path.join(d, "**", pat), recursive=True)
        if not files:
            raise SystemExit(f"no {pat} under {d}")
        for fn in files:
            for r in csv.DictReader(open(fn)):
                rows.append((int(r["Start_Timestamp"]), r.get("Stream_Id"), kind,
                             short(r[col]) if kind == "kernels" else r[col]))
    rows.sort()
    by_stream = {}
    for _, stream, kind, name in rows:
        by_stream.setdefault(stream, {"kernels": [], "copies": []})[kind].append(name)
    return by_stream


def rle(names):
    out = []
    for x in names:
        if out and out[-1][0] == x:
            out[-1][1] += 1
        else:
            out.append([x, 1])
    return " ".join(x if k == 1 else f"{x} x{k}" for x, k in out)


def compare(dir_a, dir_b, out=None):
    ta, tb = read_trace(dir_a), read_trace(dir_b)
    lines = []
    has_streams = None not in ta and None not in tb
    if has_streams:
        key = lambda t: sorted((tuple(v["kernels"]), tuple(v["copies"])) for v in t.values())
        ka, kb = key(ta), key(tb)
        equal = ka == kb
        lines.append(f"streams: {len(ka)} and {len(kb)} (matched by content; listed in sorted order)")
        for tag, k in (("A", ka), ("B", kb)):
            for i, (kern, cop) in enumerate(k):
                lines.append(f"[{tag}] stream {i}: {len(kern)} kernels, {len(cop)} copies")
                lines.append(f"[{tag}]   kernels: {rle(kern)}")
                lines.append(f"[{tag}]   copies:  {rle(cop)}")
    else:
        lines.append("the trace has no Stream_Id column: counts per kernel name and copy direction")
        count = lambda t: collections.Counter((kind, x) for v in t.values() for kind in ("kernels", "copies")
                                              for x in v[kind])
        ca, cb = count(ta), count(tb)
        equal = ca == cb
        for tag, cnt in (("A", ca), ("B", cb)):
            for (kind, x), k in sorted(cnt.items()):
                lines.append(f"[{tag}] {kind[:-1]} {x}: {k}")
    lines.append(f"A = {os.path.basename(os.path.normpath(dir_a))}, B = {os.path.basename(os.path.normpath(dir_b))}")
    lines.append("verdict: " + ("EQUAL" if equal else "DIFFERENT"))
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as f:
            f.write(text)
    sys.stdout.write(text if not out else lines[-1] + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "drive":
        drive()
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else None))
    else:
        sys.exit(__doc__)
