"""NumPy restatement of the paste rule of semtsdf_detections_to_labels (include/semtsdf.h): a detection's
mini-mask resized to its pixel box as unmold_mask does (mrcnn/utils.py:565-581: skimage resize order=1
mode="constant" without anti-aliasing, >= 0.5), every intermediate held in `dtype` (np.float32 is the
rule; np.float64 is the yardstick tests/golden/gen_paste.py measures skimage against and draws the `near`
band from), then the keep/rank/label rule through oracle.masks_to_labels on the pasted [H][W][n] masks,
which is fine at test sizes."""
import os

import numpy as np

NEAR_CAP = 1e-3  # of the box pixels; a condition on the golden's cases, not a tolerance (measured: 0.015 %)


def paste_values(mini, box, shape, dtype=np.float32):
    """The interpolated values v of one detection on the part of its box inside the image:
    (v [ch, cw] in dtype, (cy0, cx0)) or (None, None) for an empty or fully clipped box."""
    T = dtype
    H, W = int(shape[0]), int(shape[1])
    y1, x1, y2, x2 = (int(v) for v in box)
    if y2 <= y1 or x2 <= x1:
        return None, None
    cy0, cx0, cy1, cx1 = max(y1, 0), max(x1, 0), min(y2, H), min(x2, W)
    if cy1 <= cy0 or cx1 <= cx0:
        return None, None
    m = np.asarray(mini).astype(T)
    mh, mw = m.shape
    P = np.zeros((mh + 2, mw + 2), T)  # a tap outside the mini-mask reads 0
    P[1:-1, 1:-1] = m
    half = T(0.5)

    def axis(lo, hi, origin, extent, size):
        s = T(size) / T(extent)
        c = (np.arange(lo - origin, hi - origin, dtype=np.int64).astype(T) + half) * s - half
        c0 = np.floor(c)
        f = c - c0
        i = c0.astype(np.int64)
        return np.clip(i + 1, 0, size + 1), np.clip(i + 2, 0, size + 1), f

    ya, yb, fy = axis(cy0, cy1, y1, y2 - y1, mh)
    xa, xb, fx = axis(cx0, cx1, x1, x2 - x1, mw)
    fy, fx = fy[:, None], fx[None, :]
    one = T(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        top = P[ya[:, None], xa[None, :]] * (one - fx) + P[ya[:, None], xb[None, :]] * fx
        bot = P[yb[:, None], xa[None, :]] * (one - fx) + P[yb[:, None], xb[None, :]] * fx
        v = top * (one - fy) + bot * fy
    assert v.dtype == T
    return v, (cy0, cx0)


def paste_mask(mini, box, shape, dtype=np.float32):
    """bool [H, W]: v >= 0.5 at the box's pixels inside the image (a NaN is off), False elsewhere."""
    out = np.zeros((int(shape[0]), int(shape[1])), bool)
    v, at = paste_values(mini, box, shape, dtype)
    if v is not None:
        with np.errstate(invalid="ignore"):
            out[at[0]:at[0] + v.shape[0], at[1]:at[1] + v.shape[1]] = v >= dtype(0.5)
    return out


def paste_masks(boxes, minis, shape, dtype=np.float32):
    """bool [H, W, n], the detector's masks[H, W, N] as the rule makes them."""
    n = len(boxes)
    out = np.zeros((int(shape[0]), int(shape[1]), n), bool)
    for i in range(n):
        out[:, :, i] = paste_mask(minis[i], boxes[i], shape, dtype)
    return out


def near_map(boxes, minis, shape, band=1e-4):
    """bool [H, W]: pixels where some detection's f64 interpolated value lies within `band` of 0.5."""
    out = np.zeros((int(shape[0]), int(shape[1])), bool)
    for i in range(len(boxes)):
        v, at = paste_values(minis[i], boxes[i], shape, np.float64)
        if v is not None:
            with np.errstate(invalid="ignore"):
                out[at[0]:at[0] + v.shape[0], at[1]:at[1] + v.shape[1]] |= np.abs(v - 0.5) <= band
    return out


def box_pixels(boxes, shape):
    """Number of image pixels inside the boxes, summed over the boxes."""
    H, W = int(shape[0]), int(shape[1])
    t = 0
    for y1, x1, y2, x2 in np.asarray(boxes).reshape(-1, 4):
        if y2 > y1 and x2 > x1:
            t += max(min(int(y2), H) - max(int(y1), 0), 0) * max(min(int(x2), W) - max(int(x1), 0), 0)
    return t


def detections_to_labels(oracle, boxes, minis, shape, min_area=2000):
    """(labels u8 [H, W], kept, areas u32 [n]) by the rule: paste, then oracle.masks_to_labels."""
    m = paste_masks(boxes, minis, shape)
    areas = m.sum(axis=(0, 1)).astype(np.uint32)
    labels, kept = oracle.masks_to_labels(m, min_area=min_area)
    return labels, kept, areas


# ---- tests/golden/paste_golden.npz (tests/golden/gen_paste.py)
def unpack(bits, shape):
    return np.unpackbits(bits, axis=1, count=int(shape[1]), bitorder="little").astype(bool)


def golden():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "paste_golden.npz"))
    shape = tuple(int(v) for v in z["single_shape"])
    singles = [(z[f"s{k}_box"], z[f"s{k}_mini"].astype(np.float32), shape, unpack(z[f"s{k}_mask"], shape),
                unpack(z[f"s{k}_near"], shape)) for k in range(int(z["n_single"]))]
    labels = []
    for k in range(int(z["n_label"])):
        shp = tuple(int(v) for v in z[f"l{k}_shape"])
        labels.append((z[f"l{k}_boxes"], z[f"l{k}_minis"].astype(np.float32), shp, z[f"l{k}_labels"],
                       int(z[f"l{k}_kept"]), unpack(z[f"l{k}_near"], shp)))
    return singles, labels, float(z["skimage_max_dev"]), float(z["band"])


def check_golden(single_mask, label_map):
    """The golden's assertions for a producer of single masks `single_mask(box, mini, shape) -> bool
    [H, W]` and of label maps `label_map(boxes, minis, shape) -> (labels, kept)` (the restatement here,
    the device in tests/test_gpu_paste.py)."""
    singles, labels, _, _ = golden()
    assert len(singles) >= 8 and len(labels) == 2
    for k, (box, mini, shape, want, near) in enumerate(singles):
        got = single_mask(box, mini, shape)
        print(f"single {k}: box {box.tolist()} mini {mini.shape} area {int(want.sum())} near {int(near.sum())} "
              f"differing outside near {int((got != want)[~near].sum())}")
        assert int(near.sum()) <= NEAR_CAP * box_pixels(box, shape), k
        np.testing.assert_array_equal(got[~near], want[~near], err_msg=f"single {k}")
    for k, (boxes, minis, shape, want, kept, near) in enumerate(labels):
        got, got_kept = label_map(boxes, minis, shape)
        print(f"labels {k}: {shape} n {len(boxes)} kept {kept} near {int(near.sum())} "
              f"differing outside near {int((got != want)[~near].sum())}")
        assert int(near.sum()) <= NEAR_CAP * box_pixels(boxes, shape), k
        assert got_kept == kept, k
        np.testing.assert_array_equal(got[~near], want[~near], err_msg=f"labels {k}")
