"""Golden vectors of the mask paste (semtsdf_detections_to_labels), made by executing the reference's own
unmold_mask (Mask_RCNN/mrcnn/utils.py:565-581) and Mask_RCNN/dmask.py mask_detect here (run in this
container only, with the interpreter that has scikit-image 0.18.3; its OUTPUT,
tests/golden/paste_golden.npz, is what the tests read).  utils.py imports TensorFlow at module level, so
unmold_mask's text is taken from the file by name with the ast module and executed, as gen_mrcnn_utils.py
does; dmask.py is loaded as gen_masks.py does, with a stand-in model whose detect() returns the pasted
masks.

Two shims, both stated here because they decide what the golden means:
  * `np.bool = bool` (utils.py:576/579 and dmask.py:50 use the alias NumPy 1.24 removed);
  * the executed text sees a `skimage.transform.resize` with `anti_aliasing=False` bound: the reference's
    era of scikit-image had no anti-aliasing, later releases blur a downscale by default.

Mini-masks are seeded smooth sigmoid fields (a few low-frequency waves through a sigmoid, like a mask
head's output); boxes lie inside the image (unmold_mask cannot express one that crosses the border).
Per case a bit-packed `near` map marks the pixels where some detection's f64 interpolated value
(tests/paste_restatement.py in np.float64) lies within 1e-4 of 0.5: there skimage's own rounding may
decide the threshold the other way, everywhere else the masks must agree.  A case is redrawn until `near`
covers at most 0.1 % of its box pixels, and a label case until its areas differ from one another and
from the 2000-pixel rule by more than its `near` pixel count, so that neither rank nor keep can flip.

One thing skimage does that the rule does not: resize's default clip=True clips its output to the
mini-mask's own [min, max], which lifts the rim pixels that blend with the constant 0 outside up to that
minimum.  That moves no pixel across 0.5 as long as the minimum is below 0.5, which holds for a mask
head's output (background at the rim of the box); every mini-mask here is drawn with a minimum <= 0.4, and
the masks and labels are then what the reference makes, clip included.  A mini-mask that is >= 0.5
everywhere would keep its rim in the reference and lose part of it by the rule.
`skimage_max_dev` is the largest |skimage - f64 restatement clipped the same way| over 300 random boxes at
96 x 128 (upscales, downscales, one-pixel-high boxes).  The mini-masks hold fp16 values and are stored as
fp16."""
from __future__ import annotations

import ast
import functools
import importlib.util
import os
import sys
import types

import numpy as np
import skimage.transform

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import paste_restatement as PR  # noqa: E402

REF_UTILS = "/root/reference/Mask_RCNN/mrcnn/utils.py"
REF_DMASK = "/root/reference/Mask_RCNN/dmask.py"
OUT = os.path.join(HERE, "paste_golden.npz")
BAND = 1e-4
CAP = 1e-3


def load_unmold_mask():
    tree = ast.parse(open(REF_UTILS).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "unmold_mask"]
    assert len(body) == 1
    resize = functools.partial(skimage.transform.resize, anti_aliasing=False)
    ns = {"np": np, "skimage": types.SimpleNamespace(transform=types.SimpleNamespace(resize=resize))}
    exec(compile(ast.Module(body=body, type_ignores=[]), REF_UTILS, "exec"), ns)
    return ns["unmold_mask"], resize


def load_dmask():
    spec = importlib.util.spec_from_file_location("dmask_ref", REF_DMASK)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class StandInModel:
    def __init__(self, masks):
        self.masks = masks

    def detect(self, images, verbose=0):
        return [{"masks": self.masks.copy()}]


def mini_mask(rng, mh=28, mw=28, bias=1.0):
    yy, xx = np.mgrid[0:mh, 0:mw]
    yy, xx = (yy + 0.5) / mh, (xx + 0.5) / mw
    f = np.full((mh, mw), bias)
    for _ in range(4):
        f += rng.normal(0, 1.5) * np.cos(2 * np.pi * (rng.uniform(0, 1.5) * yy + rng.uniform(0, 1.5) * xx)
                                         + rng.uniform(0, 2 * np.pi))
    # fp16 values (stored as such, widened exactly): what a half-precision mask head hands over
    return (1.0 / (1.0 + np.exp(-f))).astype(np.float16).astype(np.float32)


def draw_mini(rng, mh=28, mw=28, lo=-0.5, hi=1.5):
    """A mini-mask whose smallest value is below the threshold (see the module docstring: clip)."""
    while True:
        m = mini_mask(rng, mh, mw, bias=rng.uniform(lo, hi))
        if m.min() <= 0.4:
            return m


def near_count(boxes, minis, shape):
    near = PR.near_map(boxes, minis, shape, BAND)
    return near, int(near.sum())


def single(rng, unmold, box, shape, mh, mw):
    while True:
        m = draw_mini(rng, mh, mw)
        near, k = near_count([box], [m], shape)
        if k <= CAP * PR.box_pixels([box], shape):
            break
    full = unmold(m.copy(), np.array(box), shape)  # reference code (utils.py:565-581)
    return m, np.asarray(full, bool), near


def random_box(rng, shape, lo, hi):
    H, W = shape
    h, w = int(rng.integers(lo, min(hi, H) + 1)), int(rng.integers(lo, min(hi, W) + 1))
    y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
    return [y, x, y + h, x + w]


def label_case(rng, unmold, dm, shape, n_big, n_small, big, small):
    H, W = shape
    while True:
        boxes = [random_box(rng, shape, *big) for _ in range(n_big)] + [random_box(rng, shape, *small)
                                                                        for _ in range(n_small)]
        order = rng.permutation(len(boxes))
        boxes = [boxes[i] for i in order]
        minis = [draw_mini(rng, lo=0.5, hi=2.5) for _ in boxes]
        near, k = near_count(boxes, minis, shape)
        if k > CAP * PR.box_pixels(boxes, shape):
            continue
        masks = np.stack([unmold(m.copy(), np.array(b), shape) for m, b in zip(minis, boxes)], axis=2)
        areas = np.sort(masks.sum(axis=(0, 1)))
        kept = areas[areas > 2000]
        if kept.size < 3 or kept.size == len(boxes):
            continue  # some kept, some dropped
        if np.diff(kept).min() <= k or np.abs(areas.astype(np.int64) - 2000).min() <= k:
            continue
        break
    lab = dm.mask_detect(StandInModel(masks), np.zeros((H, W, 3), np.uint8))  # reference code (dmask.py:47-59)
    return np.array(boxes, np.int32), np.stack(minis), lab.astype(np.uint8), int(kept.size), near


def skimage_deviation(rng, resize, shape=(96, 128), draws=300):
    worst = 0.0
    for d in range(draws):
        if d % 3 == 0:
            box = random_box(rng, shape, 29, 128)  # upscales
        elif d % 3 == 1:
            box = random_box(rng, shape, 2, 27)   # downscales
        else:
            box = random_box(rng, shape, 1, 128)
            box[2] = box[0] + 1                    # one pixel high
        m = draw_mini(rng)
        h, w = box[2] - box[0], box[3] - box[1]
        got = resize(m, (h, w), order=1, mode="constant")
        want, _ = PR.paste_values(m, box, shape, np.float64)
        want = np.clip(want, m.min(), m.max())  # resize's clip=True (module docstring)
        worst = max(worst, float(np.abs(got - want).max()))
    return worst


def main():
    np.bool = bool  # utils.py:576, dmask.py:50
    unmold, resize = load_unmold_mask()
    dm = load_dmask()
    rng = np.random.default_rng(2025)
    rec = {"band": np.float64(BAND)}
    shape = (96, 128)
    singles = [([10, 20, 70, 100], 28, 28), ([0, 0, 96, 128], 28, 28), ([30, 40, 58, 68], 28, 28),
               ([5, 7, 32, 34], 28, 28), ([60, 90, 89, 119], 28, 28), ([40, 50, 53, 59], 28, 28),
               ([17, 3, 18, 120], 28, 28), ([2, 77, 90, 78], 28, 28), ([50, 60, 51, 61], 28, 28),
               ([8, 16, 88, 56], 14, 20), ([70, 4, 82, 124], 14, 20)]
    for k, (box, mh, mw) in enumerate(singles):
        m, full, near = single(rng, unmold, box, shape, mh, mw)
        rec[f"s{k}_box"] = np.array(box, np.int32)
        rec[f"s{k}_mini"] = m.astype(np.float16)
        rec[f"s{k}_mask"] = np.packbits(full, axis=1, bitorder="little")
        rec[f"s{k}_near"] = np.packbits(near, axis=1, bitorder="little")
        print("single", k, box, (mh, mw), "area", int(full.sum()), "near", int(near.sum()))
    rec["n_single"] = np.int64(len(singles))
    rec["single_shape"] = np.array(shape, np.int64)
    cases = [((96, 128), 4, 4, (52, 100), (8, 40)), ((480, 640), 6, 6, (60, 400), (10, 44))]
    for k, (shp, nb, ns, big, small) in enumerate(cases):
        boxes, minis, lab, kept, near = label_case(rng, unmold, dm, shp, nb, ns, big, small)
        rec[f"l{k}_shape"] = np.array(shp, np.int64)
        rec[f"l{k}_boxes"] = boxes
        rec[f"l{k}_minis"] = minis.astype(np.float16)
        rec[f"l{k}_labels"] = lab
        rec[f"l{k}_kept"] = np.int64(kept)
        rec[f"l{k}_near"] = np.packbits(near, axis=1, bitorder="little")
        print("labels", k, shp, "n", len(boxes), "kept", kept, "near", int(near.sum()), "max label", int(lab.max()))
    rec["n_label"] = np.int64(len(cases))
    rec["skimage_max_dev"] = np.float64(skimage_deviation(rng, resize))
    print("skimage max deviation from the f64 restatement", rec["skimage_max_dev"])
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
