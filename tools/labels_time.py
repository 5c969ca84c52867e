#!/usr/bin/env python3
"""Time of the paste stage of the C5 producer (480 x 640, 100 fixed rows, the bench's calibrated fp16
model): the detector runs once on a synthetic frame, then the same (det, masks) tensors go through

  new:  MaskRCNN.labels_from (box arithmetic + class gather in torch, semtsdf_detections_to_labels)
  old:  MaskRCNN.unmold(compact=False) (grid_sample paste to masks[H, W, 100]) + semtsdf_masks_to_labels

in one process on one device.  Each path is timed three ways with HIP events on one stream: eager calls,
one captured HIP graph replayed (what GraphDetector does with the whole frame), and the C-ABI call alone
on prepared inputs.  A sample is the event time of --batch back-to-back runs divided by the batch; the
two paths alternate sample by sample; the result is the median (and minimum) of --runs samples after
--warmup.  Prints one JSON line, with the number of label pixels on which the two paths differ."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=31)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--min-area", type=int, default=2000)
    args = ap.parse_args()

    import torch

    import semtsdf
    from semtsdf import maskrcnn as MR
    from semtsdf.masks import detections_to_labels_dev, detections_to_labels_workspace, masks_to_labels_dev
    from semtsdf.synth import SyntheticStream

    lib = semtsdf.load()
    dev = torch.device("cuda", 0)
    img = torch.from_numpy(SyntheticStream(seed=1, noise=True).frame(1).rgb).to(dev)
    H, W = int(img.shape[0]), int(img.shape[1])
    cfg = MR.Config(DTYPE=torch.float16)
    model = MR.MaskRCNN(cfg, seed=0).to(dev).to(cfg.DTYPE).eval()
    model.calibrate(dev, img)
    with torch.no_grad():
        det, masks, shape, nwin = model._network(img)
    N = int(det.shape[0])
    stream = torch.cuda.current_stream(dev)
    work = torch.empty(detections_to_labels_workspace(N), dtype=torch.uint8, device=dev)
    old_labels = torch.empty((H, W), dtype=torch.uint8, device=dev)

    def new_path():
        return model.labels_from(det, masks, (H, W), shape, nwin, args.min_area, work)

    def old_path():
        out = model.unmold(det, masks, (H, W), shape, nwin, compact=False)
        masks_to_labels_dev(out["masks"].data_ptr(), W, H, N, old_labels.data_ptr(), args.min_area,
                            stream=stream.cuda_stream)
        return out

    with torch.no_grad():
        new = new_path()
        old = old_path()
        torch.cuda.synchronize()
        differ = int((new["labels"] != old_labels).sum())
        kept = int((new["areas"] > args.min_area).sum())
        detections = int((new["class_ids"] > 0).sum())

        # prepared inputs of the two C-ABI calls alone
        px, mini = new["rois"], masks[torch.arange(N, device=dev), new["class_ids"].long()].contiguous()
        full = old["masks"]
        code = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}[mini.dtype]
        lab2 = torch.empty((H, W), dtype=torch.uint8, device=dev)

        def new_call():
            detections_to_labels_dev(px.data_ptr(), mini.data_ptr(), code, int(mini.shape[1]), int(mini.shape[2]), N,
                                     W, H, lab2.data_ptr(), work.data_ptr(), args.min_area,
                                     stream=stream.cuda_stream)

        def old_call():
            masks_to_labels_dev(full.data_ptr(), W, H, N, old_labels.data_ptr(), args.min_area,
                                stream=stream.cuda_stream)

        def graph_of(fn):
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(3):
                    fn()
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                keep = fn()
            return g, keep

        def sample(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.batch):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / args.batch  # microseconds per run

        def ab(a, b):
            ta, tb = [], []
            for k in range(args.warmup + args.runs):
                x, y = sample(a), sample(b)
                if k >= args.warmup:
                    ta.append(x)
                    tb.append(y)
            return ta, tb

        def stat(ts):
            return {"median_us": round(statistics.median(ts), 2), "min_us": round(min(ts), 2)}

        res = {}
        ta, tb = ab(new_path, old_path)
        res["eager"] = {"new": stat(ta), "old": stat(tb)}
        # the old path as the bench runs it: unmold inside the graph, semtsdf_masks_to_labels (which
        # allocates its scratch) after the replay
        gn, _kn = graph_of(new_path)
        go, ko = graph_of(lambda: model.unmold(det, masks, (H, W), shape, nwin, compact=False))

        def old_replay():
            go.replay()
            masks_to_labels_dev(ko["masks"].data_ptr(), W, H, N, old_labels.data_ptr(), args.min_area,
                                stream=stream.cuda_stream)

        ta, tb = ab(gn.replay, old_replay)
        res["graph"] = {"new": stat(ta), "old": stat(tb)}
        ta, tb = ab(new_call, old_call)
        res["abi_call_alone"] = {"new_detections_to_labels": stat(ta), "old_masks_to_labels": stat(tb)}
        torch.cuda.synchronize()
    print(json.dumps({
        "tool": "labels_time", "image": [H, W], "rows": N, "mini": list(mini.shape[1:]), "mini_dtype": str(mini.dtype),
        "detections": detections, "kept": kept, "min_area": args.min_area, "label_pixels_differing": differ,
        "runs": args.runs, "batch": args.batch, "warmup": args.warmup, **res,
        "graph_speedup": round(res["graph"]["old"]["median_us"] / res["graph"]["new"]["median_us"], 2),
        "old_masks_bytes": int(np.prod(full.shape)), "build_key": lib.semtsdf_build_key().decode()[:16],
    }), flush=True)


if __name__ == "__main__":
    main()
