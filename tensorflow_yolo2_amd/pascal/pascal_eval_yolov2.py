"""VOC mAP of the YOLOv2 anchor detector over an image set (not in the reference, which has no evaluation code):
    python -m tensorflow_yolo2_amd.pascal.pascal_eval_yolov2 --devkit data/VOCdevkit --image-set test \
        [--weights FILE | --ckpt-dir DIR] [--size 416] [--batch 32] [--metric 07|10]
The shape is pascal_eval_darknet.py's.  The images come from the device-resident pool in list order; per batch, four
calls on one stream and nothing on the host:
    DeviceVOC.eval_batch (resize) -> YOLOv2Detector.detect_batch = forward on the uint8 batch (moving statistics) ->
    y2_detect_anchor_batch (anchor decode, class choice, boxes in the pixels of each original image, class-aware NMS:
    one launch from the raw head) -> y2_voc_match_batch (TP / FP / ignored against the image's ground truth)
The det / score / count / flags of every batch land in ONE device buffer; after the last batch it is copied to the host
once and utils/detect_batch.map_from_flags makes the per-class curves and the APs.  A detection is an anchor's box with
its best class (score = objectness * class probability): one row per anchor, not one per class as Darknet's `valid`
writes.  The anchors and the class count are the snapshot's (pascal_train_yolov2.py); with neither --weights nor
--ckpt-dir the initial values are evaluated with the published VOC anchors: a plumbing run."""
import argparse
import sys

import numpy as np
import torch

from .. import engine
from ..img_dataset import pascal_voc
from ..utils import detect_batch
from ..yolo2_nets import net_utils, yolov2


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--devkit", required=True, help="VOCdevkit directory (cfg.PASCAL_PATH)")
    ap.add_argument("--image-set", default="test")
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--weights", default=None, help="snapshot file (train_iter_<i>.npz of pascal_train_yolov2.py)")
    ap.add_argument("--ckpt-dir", default=None, help="directory of train_iter_*.npz snapshots: the latest is evaluated")
    ap.add_argument("--thresh", type=float, default=0.005, help="score above which a box is a detection")
    ap.add_argument("--nms", type=float, default=0.45, help="IoU above which a box of the same class is suppressed")
    ap.add_argument("--max-out", type=int, default=100, help="detections kept per image")
    ap.add_argument("--metric", default="07", choices=("07", "10"), help="07: 11-point AP; 10: area under the envelope")
    ap.add_argument("--width-div", type=int, default=1, help="divide every inner width (tests)")
    ap.add_argument("--keep-grids", action="store_true", help="return the raw head outputs of every image (tests)")
    args = ap.parse_args(argv)
    if args.size < 32 or args.size % 32:
        ap.error("--size %d: the detector head needs a positive multiple of 32 (S = size / 32)" % args.size)
    if (args.size // 32) ** 2 * len(yolov2.ANCHORS_VOC) > 2048:
        ap.error("--size %d: more than 2048 candidates per image" % args.size)
    if args.batch < 1 or args.max_out < 1 or args.width_div < 1:
        ap.error("--batch, --max-out and --width-div must be at least 1")
    return args


def main(argv=None):
    args = parse_args(argv)
    from ..img_dataset.device_voc import DeviceVOC
    imdb = DeviceVOC(args.image_set, batch_size=args.batch, devkit_path=args.devkit, flipped=False)
    snapshot = args.weights
    if not snapshot and args.ckpt_dir:
        sfiles = net_utils.get_ordered_yolov2_ckpts(args.ckpt_dir)
        snapshot = sfiles[-1] if sfiles else None
    anchors, num_class = yolov2.ANCHORS_VOC, imdb.num_class
    if snapshot:
        anchors, num_class, _it = net_utils.read_yolov2_meta(snapshot)
        if num_class != imdb.num_class:
            raise ValueError("snapshot %s: num_class is %d, the image set has %d" % (snapshot, num_class, imdb.num_class))
    detector = yolov2.YOLOv2Detector(args.batch, args.size, num_class=num_class, anchors=anchors, dtype=args.dtype,
                                     width_div=args.width_div)
    restored = 0
    if snapshot:
        print('Restorining model from weight file {:s}'.format(snapshot))
        restored = net_utils.restore_yolov2_variables(detector, snapshot)
    result = evaluate_yolov2(detector, imdb, args.size, args.thresh, args.nms, args.max_out, args.metric == "07",
                             args.keep_grids)
    for c in sorted(result["aps"]):
        print('AP for {:s} = {:.4f}'.format(pascal_voc.CLASSES[c], result["aps"][c]))
    print('Mean AP = {:.4f} ({:d} images, {:d} detections, VOC{:s} metric)'.format(
        result["mAP"], len(imdb.entries), len(result["rows"]["flag"]), "07" if args.metric == "07" else "10+"))
    result.update(restored=restored, detector=detector, imdb=imdb)
    return result


def evaluate_yolov2(detector, imdb, size, thresh=0.005, nms=0.45, max_out=100, use_07_metric=True, keep_grids=False):
    """one pass over imdb's image list through `detector` (a YOLOv2Detector of imdb.batch_size images of `size`):
    {"mAP", "aps", "rows", "count", "npos"[, "grids"]} as pascal_eval_darknet.evaluate; everything per image runs on the
    device, one copy at the end"""
    n = imdb.batch_size
    assert detector.batch == n and detector.size == size, (detector.batch, detector.size, n, size)
    S, B, D = detector.S, detector.B, 5 + detector.num_class
    entries = len(imdb.entries)
    batches = (entries + n - 1) // n
    N = batches * n
    # det [N][max_out][6] | score [N][max_out] (float bits) | flags [N][max_out] | count [N]: one buffer, one copy
    words = N * max_out * 8 + N
    acc = torch.empty(words, dtype=torch.int32, device="cuda")
    det = acc[:N * max_out * 6].view(N, max_out, 6)
    score = acc[N * max_out * 6:N * max_out * 7].view(torch.float32).view(N, max_out)
    flags = acc[N * max_out * 7:N * max_out * 8].view(N, max_out)
    count = acc[N * max_out * 8:]
    grids = torch.empty((N, S, S, B, D), dtype=torch.float32, device="cuda") if keep_grids else None
    difficult = imdb.difficult
    for k in range(batches):
        lo = k * n
        images, _valid = imdb.eval_batch(size, lo)
        detector.detect_batch(images, imdb.table, imdb.eval_index, thresh, nms, max_out,
                              out=(det[lo:lo + n], score[lo:lo + n], count[lo:lo + n]),
                              grid_out=grids[lo:lo + n] if grids is not None else None)
        engine.voc_match_batch(det[lo:lo + n], score[lo:lo + n], count[lo:lo + n], imdb.boxes, imdb.counts, difficult,
                               imdb.eval_index, 0.5, out=flags[lo:lo + n])
    host = acc.cpu().numpy()                                  # the one device-to-host copy (it waits for the stream)
    det_h = host[:N * max_out * 6].reshape(N, max_out, 6)[:entries]
    score_h = host[N * max_out * 6:N * max_out * 7].view(np.float32).reshape(N, max_out)[:entries]
    flags_h = host[N * max_out * 7:N * max_out * 8].reshape(N, max_out)[:entries]
    count_h = host[N * max_out * 8:][:entries]
    live = np.arange(max_out)[None, :] < count_h[:, None]      # image order, each image's rows in descending score
    rows = {"image": np.nonzero(live)[0], "box": det_h[live][:, :4], "class": det_h[live][:, 4],
            "candidate": det_h[live][:, 5], "score": score_h[live], "flag": flags_h[live]}
    npos = detect_batch.npos_from_objects([o[4] for e in imdb.entries for o in e['objs']],
                                          [d for e in imdb.entries for d in e['difficult']])
    mAP, aps = detect_batch.map_from_flags((rows["class"], rows["score"], rows["flag"]), npos,
                                           use_07_metric=use_07_metric)
    result = {"mAP": mAP, "aps": aps, "rows": rows, "count": count_h.copy(), "npos": npos}
    if grids is not None:
        result["grids"] = grids[:entries]
    return result


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
