"""COCO AP / AR of the YOLOv2 anchor detector over the images of an instances file (not in the reference, which has no
evaluation code):
    python -m tensorflow_yolo2_amd.coco.coco_eval_yolov2 --annotations instances_val2014.json --images val2014 \
        [--image-list 5k.txt] --cfg yolov2.cfg --darknet-weights yolov2.weights [--names coco.names] [--size 416]
        [--batch 32] [--letterbox [--fill 127]] [--protocol repo|darknet] [--results FILE.json]
The shape is pascal_eval_yolov2.py's.  The images come from the device-resident pool in ascending image id; per batch,
four calls on one stream and nothing on the host:
    DeviceCOCO.eval_batch (resize) -> YOLOv2Detector.detect_classes_batch = forward on the batch (moving statistics) and
    one row per (candidate, class) whose score passes, each class ordered and walked on its own, as Darknet's `valid` writes
    them -> y2_coco_match_batch over the (image, class) segments: COCO's matching under its ten IoU thresholds and four
    area ranges at once, one packed word per row and area range
The det / score / match / count of every batch land in ONE device buffer; after the last batch it is copied to the host
once, and utils/coco_eval.accumulate and summarize make the precision / recall arrays and the twelve numbers, printed in
COCO's wording.  --letterbox, --fill and --protocol follow pascal_eval_yolov2.py's rules: --protocol darknet scores the
float rows of Darknet's own letterbox, un-map and NMS (it implies --letterbox and needs the darknet topology).
The model's class count -- the cfg's, or the snapshot's -- must be the file's category count, and the line count of
--names likewise: the categories are taken in ascending id, which with the published files is the order of coco.names.
--results FILE.json writes the rows as Darknet's `valid` writes them for COCO (utils/coco_eval.write_results)."""
import argparse
import sys

import numpy as np
import torch

from .. import engine
from ..pascal import yolov2_model_flags as model_flags
from ..utils import coco_eval

ROW_BYTES = 4 * (6 + 1 + len(coco_eval.AREA_RANGES))      # det, score and the match words of one row of the buffer


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--annotations", required=True, help="a COCO instances JSON file (instances_val2014.json)")
    ap.add_argument("--images", required=True, help="the directory that holds the file_name of every image")
    ap.add_argument("--image-list", default=None,
                    help="a Darknet list file (5k.txt): only the images whose file name is the base name of a listed path")
    model_flags.add_model_flags(ap, 32, None, "evaluated", "the file's category count")
    ap.add_argument("--thresh", type=float, default=0.005, help="score above which a box is a detection")
    ap.add_argument("--nms", type=float, default=0.45, help="IoU above which a box of the same class is suppressed")
    ap.add_argument("--max-per-class", type=int, default=100,
                    help="rows kept per image and class.  100 is COCO's maxDets, so the default loses nothing.  The device "
                         "buffer takes %d bytes per row, images x classes x this many rows: about %.1f GB for 5,000 "
                         "images of 80 classes at the default" % (ROW_BYTES, 5000 * 80 * 100 * ROW_BYTES / 1e9))
    ap.add_argument("--letterbox", action="store_true",
                    help="keep every image's aspect ratio: embed it in the square input between bars of --fill and "
                         "un-map the boxes from that rectangle, as Darknet's test-time input (default: a plain stretch)")
    ap.add_argument("--fill", type=int, default=None, help="with --letterbox: the value of the bars, 0..255 (127)")
    ap.add_argument("--protocol", default="repo", choices=("repo", "darknet"),
                    help="darknet: Darknet's test-time protocol -- its float letterbox with bars of 0.5, its float un-map "
                         "and NMS, float corners in the rows and the results file.  Implies --letterbox; needs "
                         "--darknet-weights or --cfg; not with --fill (default: this repository's integer-pixel protocol)")
    ap.add_argument("--results", default=None, metavar="FILE.json",
                    help="write the rows there as Darknet's `valid` writes them for COCO: image_id, the original "
                         "category_id, bbox = x, y, w, h and score")
    model_flags.add_test_flags(ap)
    args = ap.parse_args(argv)
    args.error = ap.error
    model_flags.resolve_cfg(ap, args)
    model_flags.check_size(ap, args)
    if args.batch < 1 or args.width_div < 1 or args.max_per_class < 1:
        ap.error("--batch, --max-per-class and --width-div must be at least 1")
    if args.protocol == "darknet":
        if args.fill is not None:
            ap.error("--fill is not read with --protocol darknet: Darknet's bars are 0.5")
        if not (args.darknet_weights or args.cfg):
            ap.error("--protocol darknet needs the darknet topology (--darknet-weights FILE): the paper topology's input "
                     "is BGR in [-1, 1)")
        args.letterbox = True
    if args.fill is None:
        args.fill = 127
    if not 0 <= args.fill <= 255:
        ap.error("--fill %d outside 0..255" % args.fill)
    model_flags.check_weights(ap, args)
    return args


def main(argv=None):
    args = parse_args(argv)
    from ..img_dataset.device_coco import DeviceCOCO
    try:
        imdb = DeviceCOCO(args.annotations, args.images, args.batch, image_list=args.image_list)
    except (OSError, ValueError) as e:
        args.error("--annotations: %s" % e)
    snapshot, anchors, num_class, bn_eps = model_flags.find_snapshot(args, imdb.num_class)
    if num_class != imdb.num_class:
        args.error("the model (%s) has %d classes, %s has %d categories"
                   % (args.cfg or snapshot, num_class, args.annotations, imdb.num_class))
    model_flags.class_names(args.error, args, num_class, imdb.classes)
    detector, restored = model_flags.build_detector(args, snapshot, anchors, num_class, bn_eps)
    result = evaluate_coco(detector, imdb, args.size, args.thresh, args.nms, args.max_per_class, args.keep_grids,
                           args.letterbox, args.fill, protocol=args.protocol)
    for line in coco_eval.summary_lines(result["stats"]):
        print(line)
    print('{:d} images, {:d} detections; {:d} of {:d} (image, class) segments reached --max-per-class {:d}'.format(
        len(imdb.entries), len(result["rows"]["score"]), result["saturated"], result["count"].size, args.max_per_class))
    if args.results:
        result["results_file"] = coco_eval.write_results(args.results, result["rows"], imdb.dataset)
    result.update(restored=restored, detector=detector, imdb=imdb, topology=detector.topology)
    return result


def evaluate_coco(detector, imdb, size, thresh=0.005, nms=0.45, max_per_class=100, keep_grids=False, letterbox=False,
                  fill=127, protocol="repo"):
    """one pass over imdb's images (a DeviceCOCO) through `detector` (a YOLOv2Detector of imdb.batch_size images of `size`)
    -> {"stats" the twelve numbers of coco_eval.summarize, "precision", "recall", "rows" (coco_eval's dict, with "box" the
    rows' own four words and "candidate"), "count" [entries][num_class], "saturated"[, "grids"]}; everything per image
    runs on the device, one copy at the end.  An image is num_class segments of max_per_class rows.  letterbox: the batches
    are letterboxed between bars of `fill` and the boxes un-mapped from each picture's rectangle.  protocol="darknet":
    Darknet's test-time protocol (csrc/darknet_io.hip) -- letterboxed by definition (letterbox must be set), a detector of
    a Darknet topology, the default `fill`; the matcher then reads float rows (row_form 1)"""
    if protocol not in ("repo", "darknet"):
        raise ValueError("protocol %r is neither 'repo' nor 'darknet'" % (protocol,))
    darknet = protocol == "darknet"
    if darknet and not letterbox:
        raise ValueError("protocol='darknet' scores a letterboxed input: letterbox=True")
    if darknet and getattr(detector, "topology", "paper") not in ("darknet", "tiny"):
        raise ValueError("protocol='darknet' needs a detector of the \"darknet\" topology, not %r"
                         % (getattr(detector, "topology", "paper"),))
    if detector.num_class != imdb.num_class:
        raise ValueError("the detector has %d classes, the annotations have %d categories"
                         % (detector.num_class, imdb.num_class))
    row_form = 1 if darknet else 0
    n = imdb.batch_size
    assert detector.batch == n and detector.size == size, (detector.batch, detector.size, n, size)
    S, B, D = detector.S, detector.B, 5 + detector.num_class
    entries = len(imdb.entries)
    batches = (entries + n - 1) // n
    segs, R, A = detector.num_class, max_per_class, len(coco_eval.AREA_RANGES)
    N = batches * n * segs
    # det [N][R][6] | score [N][R] (float bits) | match [N][R][A] | count [N]: one buffer, one copy
    words = N * R * (7 + A) + N
    acc = torch.empty(words, dtype=torch.int32, device="cuda")
    det = acc[:N * R * 6].view(N, R, 6)
    score = acc[N * R * 6:N * R * 7].view(torch.float32).view(N, R)
    match = acc[N * R * 7:N * R * (7 + A)].view(N, R, A)
    count = acc[N * R * (7 + A):]
    grids = torch.empty((batches * n, S, S, B, D), dtype=torch.float32, device="cuda") if keep_grids else None
    seg_index = torch.empty(n * segs, dtype=torch.int32, device="cuda")
    thresholds = torch.as_tensor(coco_eval.THRESHOLDS).cuda()
    area_ranges = torch.as_tensor(coco_eval.AREA_RANGES).cuda()
    for k in range(batches):
        lo, m = k * n * segs, n * segs
        images, _valid = imdb.eval_batch(size, k * n, letterbox=letterbox, fill=fill, protocol=protocol)
        out = (det[lo:lo + m], score[lo:lo + m], count[lo:lo + m])
        detector.detect_classes_batch(images, imdb.table, imdb.eval_index, thresh, nms, max_per_class, out=out,
                                      grid_out=grids[k * n:k * n + n] if grids is not None else None,
                                      letterbox=letterbox, protocol=protocol)
        seg_index.view(n, segs).copy_(imdb.eval_index[:n, None].expand(n, segs))     # on the device: nothing waits
        engine.coco_match_batch(det[lo:lo + m], count[lo:lo + m], imdb.boxes, imdb.area, imdb.crowd, imdb.counts,
                                seg_index, thresholds, area_ranges, row_form, out=match[lo:lo + m])
    host = acc.cpu().numpy()                                  # the one device-to-host copy (it waits for the stream)
    live_segs = entries * segs
    det_h = host[:N * R * 6].reshape(N, R, 6)[:live_segs]
    score_h = host[N * R * 6:N * R * 7].view(np.float32).reshape(N, R)[:live_segs]
    match_h = host[N * R * 7:N * R * (7 + A)].reshape(N, R, A)[:live_segs]
    count_h = host[N * R * (7 + A):][:live_segs]
    live = np.arange(R)[None, :] < count_h[:, None]            # image order, then class, each segment in descending score
    rows_h = det_h[live]
    box = np.ascontiguousarray(rows_h[:, :4])
    rows = {"image": np.nonzero(live)[0] // segs, "box": box.view(np.float32) if darknet else box,
            "class": rows_h[:, 4], "candidate": rows_h[:, 5], "score": score_h[live], "match": match_h[live],
            "bbox": coco_eval.row_xywh(rows_h, row_form)}
    precision, recall = coco_eval.accumulate(rows, imdb.dataset)
    result = {"stats": coco_eval.summarize(precision, recall), "precision": precision, "recall": recall, "rows": rows,
              "count": count_h.reshape(entries, segs).copy(), "saturated": int((count_h >= max_per_class).sum())}
    if grids is not None:
        result["grids"] = grids[:entries]
    return result


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
