"""The YOLOv2 anchor detector on plain image files (not in the reference, whose detect script is the grid model's):
    python -m tensorflow_yolo2_amd.pascal.pascal_detect_yolov2 [--weights FILE | --ckpt-dir DIR | --darknet-weights FILE]
        --images A.jpg B.jpg ...
        [--size 416] [--thresh 0.24] [--nms 0.45] [--stretch] [--out FILE]
The files are decoded once into ONE device pool (img_dataset/device_images.py); per batch, DeviceImages.batch makes the
letterboxed input -- every image keeps its aspect ratio between bars of --fill, as at Darknet's test time -- and
YOLOv2Detector.detect_batch runs the forward pass and ONE detect launch that decodes, un-maps the boxes from each
picture's rectangle and does the class-aware NMS (y2_detect_anchor_batch_lb).  --stretch is the evaluator's default
instead: a plain resize.  One line per detection, `image class score xmin ymin xmax ymax`, in the 1-based pixels of each
ORIGINAL image, images in the order given and each image's rows in descending score.  Drawing boxes is not part of it.
The anchors and the class count are the snapshot's; with neither --weights nor --ckpt-dir the initial values run: a
plumbing run.  --darknet-weights FILE runs a file Darknet wrote for yolov2-voc.cfg instead: the "darknet" topology of
yolo2_nets/yolov2.py with the published VOC anchors (net_utils.load_darknet_weights); every other flag works as before."""
import argparse
import sys

import torch

from ..img_dataset import pascal_voc
from ..yolo2_nets import net_utils, yolov2


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", nargs="+", required=True, help="image files")
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--batch", type=int, default=None, help="images per forward pass (default: all of them, at most 32)")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--weights", default=None, help="snapshot file (train_iter_<i>.npz of pascal_train_yolov2.py)")
    ap.add_argument("--ckpt-dir", default=None, help="directory of train_iter_*.npz snapshots: the latest is used")
    ap.add_argument("--darknet-weights", default=None,
                    help="a Darknet .weights file of yolov2-voc.cfg (yolov2-voc.weights): builds the \"darknet\" topology "
                         "with the published VOC anchors and 20 classes; not with --weights or --ckpt-dir")
    ap.add_argument("--thresh", type=float, default=0.24, help="score above which a box is a detection")
    ap.add_argument("--nms", type=float, default=0.45, help="IoU above which a box of the same class is suppressed")
    ap.add_argument("--max-out", type=int, default=100, help="detections kept per image")
    ap.add_argument("--stretch", action="store_true", help="resize without keeping the aspect ratio (no letterbox)")
    ap.add_argument("--fill", type=int, default=127, help="the value of the letterbox bars, 0..255")
    ap.add_argument("--out", default=None, help="write the lines to this file as well")
    ap.add_argument("--width-div", type=int, default=1, help="divide every inner width (tests)")
    ap.add_argument("--keep-grids", action="store_true", help="return the raw head outputs of every image (tests)")
    args = ap.parse_args(argv)
    if args.size < 32 or args.size % 32:
        ap.error("--size %d: the detector head needs a positive multiple of 32 (S = size / 32)" % args.size)
    if (args.size // 32) ** 2 * len(yolov2.ANCHORS_VOC) > 2048:
        ap.error("--size %d: more than 2048 candidates per image" % args.size)
    if args.batch is None:
        args.batch = min(len(args.images), 32)
    if args.batch < 1 or args.max_out < 1 or args.width_div < 1:
        ap.error("--batch, --max-out and --width-div must be at least 1")
    if not 0 <= args.fill <= 255:
        ap.error("--fill %d outside 0..255" % args.fill)
    if args.darknet_weights and (args.weights or args.ckpt_dir):
        ap.error("--darknet-weights goes with neither --weights nor --ckpt-dir")
    return args


def main(argv=None):
    args = parse_args(argv)
    from ..img_dataset.device_images import DeviceImages
    pool = DeviceImages(args.images, args.batch)
    snapshot = args.weights
    if not snapshot and args.ckpt_dir:
        sfiles = net_utils.get_ordered_yolov2_ckpts(args.ckpt_dir)
        snapshot = sfiles[-1] if sfiles else None
    anchors, num_class = yolov2.ANCHORS_VOC, len(pascal_voc.CLASSES)
    bn_eps = None
    if snapshot:
        anchors, num_class, _it = net_utils.read_yolov2_meta(snapshot)
        bn_eps = net_utils.read_yolov2_bn_eps(snapshot)
    detector = yolov2.YOLOv2Detector(args.batch, args.size, num_class=num_class, anchors=anchors, dtype=args.dtype,
                                     width_div=args.width_div, bn_eps=bn_eps,
                                     topology="darknet" if args.darknet_weights else "paper")
    restored = 0
    if args.darknet_weights:
        print('Restorining model from Darknet weight file {:s}'.format(args.darknet_weights))
        seen = net_utils.load_darknet_weights(detector, args.darknet_weights)
        print('{:d} images seen'.format(seen))
    if snapshot:
        print('Restorining model from weight file {:s}'.format(snapshot))
        restored = net_utils.restore_yolov2_variables(detector, snapshot)
    names = pascal_voc.CLASSES if num_class == len(pascal_voc.CLASSES) else [str(c) for c in range(num_class)]
    n, entries = args.batch, len(pool.entries)
    grids = []
    rows = []
    for start in range(0, entries, n):
        images, valid = pool.batch(args.size, start, letterbox=not args.stretch, fill=args.fill)
        grid_out = None
        if args.keep_grids:
            grid_out = torch.empty((n, detector.S, detector.S, detector.B, 5 + num_class), dtype=torch.float32,
                                   device="cuda")
            grids.append(grid_out)
        det, score, count = detector.detect_batch(images, pool.table, pool.eval_index, args.thresh, args.nms,
                                                  args.max_out, grid_out=grid_out, letterbox=not args.stretch)
        det, score, count = det.cpu().numpy(), score.cpu().numpy(), count.cpu().numpy()
        for k in range(valid):
            for d, s in zip(det[k, :count[k]], score[k, :count[k]]):
                rows.append((pool.paths[start + k], names[d[4]], float(s), int(d[0]), int(d[1]), int(d[2]), int(d[3])))
    lines = ["%s %s %.6f %d %d %d %d" % r for r in rows]
    for line in lines:
        print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(line + "\n" for line in lines))
    result = {"rows": rows, "restored": restored, "detector": detector, "pool": pool}
    if args.keep_grids:
        result["grids"] = torch.cat(grids)[:entries]
    return result


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
