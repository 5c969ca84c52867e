"""Golden words of the tracking restatements (tests/icp_restatement.py, pyramid_restatement.py,
rgbd_restatement.py): what restate_system, restate_system_level and restate_rgbd_system say on the
cases of the tracking tests, as int64 words.  Its OUTPUT, tests/golden/track_words_golden.npz, pins
the definitions themselves: it was written by the restatements as they stood before their shared
projection and word packing were factored out, and tests/test_track_words_golden.py recomputes it.

Integers only: the sums are of RN(a b 2^k) terms formed in float64 from f32 factors, so they do not
depend on the machine.  The loops over these words go through LAPACK and are not pinned here.

Cases (cases() below, the test calls it too):
  field_mw{0,1}_s{1,2}   restate_system on the ragged field case (icp_restatement.field_case, restated
                         frame maps) against the view's maps at min_weight 0 and 1, stride 1 and 2
  scene                  restate_system on the tracking scene at E_ref
  level{1,2}_s{1,2}      restate_system_level on levels 1 and 2 of scene_pyramid() with the gates of
                         their entry of semtsdf.track.PYRAMID_SCHEDULE, stride 1 and 2
  rgbd_l{0,1}_s{1,2}     restate_rgbd_system on field_inputs(level) with FIELD_GATES, all 64 words
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "slam-maskrcnn_amd"), os.path.join(ROOT, "oracle"), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, "track_words_golden.npz")


def cases():
    """{name: int64 words} of every pinned case."""
    import icp_restatement as I
    import model_maps_restatement as R
    import pyramid_restatement as P
    import rgbd_restatement as G
    from semtsdf.track import PYRAMID_SCHEDULE

    out = {}
    eye = np.eye(4, dtype=np.float32)
    p, _, _, depth = I.field_case()
    fm = I.restate_frame_maps(depth, list(p.Kinv), p.depth_scale)
    for mw in (0, 1):
        m = R.field_view(0x3, mw)[4]
        for stride in (1, 2):
            out[f"field_mw{mw}_s{stride}"] = I.restate_system(fm, m, list(p.K), eye, I.field_offset(), stride=stride,
                                                               **I.FIELD_GATES)
    sc = I.tracking_scene()
    out["scene"] = I.scene_system(sc["E_ref"])
    pyr = P.scene_pyramid()
    gates = {int(level): (dist_max, cos_min) for level, _, dist_max, cos_min in PYRAMID_SCHEDULE}
    for level in (1, 2):
        for stride in (1, 2):
            out[f"level{level}_s{stride}"] = P.restate_system_level(pyr[level], sc["model"], list(sc["p"].K), sc["E_ref"],
                                                                    sc["E_ref"], *gates[level], stride)
    for level in (0, 1):
        fp, frame, m, f_int, m_int = G.field_inputs(level)
        for stride in (1, 2):
            out[f"rgbd_l{level}_s{stride}"] = G.restate_rgbd_system(frame, m, f_int, m_int, level, list(fp.K), eye,
                                                                    I.field_offset(), stride=stride, **G.FIELD_GATES)
    return {k: np.asarray(v, np.int64) for k, v in out.items()}


def main():
    out = cases()
    np.savez_compressed(OUT, **out)
    for k, v in out.items():
        print(f"{k:<16}{v.size:>4} words, counts {v[28:32].tolist()}" + (f" / {v[60:64].tolist()}" if v.size == 64 else ""))
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
