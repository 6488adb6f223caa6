"""The YOLOv2 anchor detector on plain image files (not in the reference, whose detect script is the grid model's):
    python -m tensorflow_yolo2_amd.pascal.pascal_detect_yolov2 [--weights FILE | --ckpt-dir DIR | --darknet-weights FILE]
        [--cfg FILE] [--names FILE]
        --images A.jpg B.jpg ...
        [--size 416] [--thresh 0.24] [--nms 0.45] [--stretch] [--protocol repo|darknet] [--out FILE]
The files are decoded once into ONE device pool (img_dataset/device_images.py); per batch, DeviceImages.batch makes the
letterboxed input -- every image keeps its aspect ratio between bars of --fill, as at Darknet's test time -- and
YOLOv2Detector.detect_batch runs the forward pass and ONE detect launch that decodes, un-maps the boxes from each
picture's rectangle and does the class-aware NMS (y2_detect_anchor_batch_lb).  --stretch is the evaluator's default
instead: a plain resize.  One line per detection, `image class score xmin ymin xmax ymax`, in the 1-based pixels of each
ORIGINAL image, images in the order given and each image's rows in descending score.  Drawing boxes is not part of it.
The anchors and the class count are the snapshot's; with neither --weights nor --ckpt-dir the initial values run: a
plumbing run.  --protocol darknet prints what Darknet's own detector would: the float letterbox with bars of 0.5
(y2_letterbox_darknet_batch), one line per (box, class) row above --thresh after a per-class float NMS
(y2_detect_anchor_classes_batch_dk; at most --max-out rows per class), float corners, every number with "%f"; each image's
rows class by class, each class in descending score.  It needs --darknet-weights and goes with neither --stretch nor
--fill.  --darknet-weights FILE runs a file Darknet wrote for yolov2-voc.cfg instead: the "darknet" topology of
yolo2_nets/yolov2.py with the published VOC anchors (net_utils.load_darknet_weights); every other flag works as before.
A file of tiny-yolo-voc.cfg is taken the same way: its float count says so (net_utils.darknet_file_topology), and the
"tiny" topology is built with that graph's published anchors.  --cfg FILE names the Darknet cfg that goes with the
`.weights` file instead: the graph, the class count, the anchors and the widths are the file's (utils/darknet_cfg.py;
YOLOv2Detector.from_cfg), so the COCO models load -- `--cfg yolov2.cfg --darknet-weights yolov2.weights --names coco.names`
-- and --names FILE writes each detection under its class name (one per line; the count must be the model's).  --tree FILE
(or softmax_tree= of --cfg) runs a word-tree model: a detection is the node where the walk down the tree stops at
--hier-thresh (tree_thresh of --cfg, else 0.5), written under --names, else under the tree's label of that node.
YOLO9000 loads the same way -- `--cfg yolo9000.cfg --darknet-weights yolo9000.weights --names 9k.names` -- with its
28,269-filter last layer run by engine.WideHead (--dtype f16 or fp8; `tree=` found next to the cfg or given as --tree; `map=`
is not read).  On such a wide model --protocol darknet takes YOLOv2Detector.detect_tree_batch: a candidate has one class,
its node, so the rows are one flat list per image in descending score (y2_detect_anchor_tree_batch_dk; at most --max-out
rows per image) in the same line format."""
import argparse
import sys

import torch

from ..img_dataset import pascal_voc
from . import yolov2_model_flags as model_flags


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", nargs="+", required=True, help="image files")
    model_flags.add_model_flags(ap, None, "images per forward pass (default: all of them, at most 32)", "used",
                                "20 classes")
    ap.add_argument("--thresh", type=float, default=0.24, help="score above which a box is a detection")
    ap.add_argument("--nms", type=float, default=0.45, help="IoU above which a box of the same class is suppressed")
    ap.add_argument("--max-out", type=int, default=100, help="detections kept per image")
    ap.add_argument("--stretch", action="store_true", help="resize without keeping the aspect ratio (no letterbox)")
    ap.add_argument("--fill", type=int, default=None, help="the value of the letterbox bars, 0..255 (127)")
    ap.add_argument("--protocol", default="repo", choices=("repo", "darknet"),
                    help="darknet: Darknet's float letterbox, un-map and per-class NMS; one line per (box, class) row with "
                         "float corners.  Needs --darknet-weights; not with --stretch or --fill")
    ap.add_argument("--out", default=None, help="write the lines to this file as well")
    model_flags.add_test_flags(ap)
    args = ap.parse_args(argv)
    args.error = ap.error
    model_flags.resolve_cfg(ap, args, wide_head=True)
    model_flags.check_size(ap, args)
    if args.batch is None:
        args.batch = min(len(args.images), 32)
    if args.batch < 1 or args.max_out < 1 or args.width_div < 1:
        ap.error("--batch, --max-out and --width-div must be at least 1")
    if args.protocol == "darknet":
        if args.stretch:
            ap.error("--protocol darknet is letterboxed: not with --stretch")
        if args.fill is not None:
            ap.error("--fill is not read with --protocol darknet: Darknet's bars are 0.5")
        if not (args.darknet_weights or args.cfg):
            ap.error("--protocol darknet needs the darknet topology (--darknet-weights FILE): the paper topology's input "
                     "is BGR in [-1, 1)")
    if args.fill is None:
        args.fill = 127
    if not 0 <= args.fill <= 255:
        ap.error("--fill %d outside 0..255" % args.fill)
    model_flags.check_weights(ap, args)
    return args


def main(argv=None):
    args = parse_args(argv)
    from ..img_dataset.device_images import DeviceImages
    pool = DeviceImages(args.images, args.batch)
    snapshot, anchors, num_class, bn_eps = model_flags.find_snapshot(args, len(pascal_voc.CLASSES))
    detector, restored = model_flags.build_detector(args, snapshot, anchors, num_class, bn_eps)
    names = pascal_voc.CLASSES if num_class == len(pascal_voc.CLASSES) else [str(c) for c in range(num_class)]
    if args.tree_record is not None:          # a word tree: a detection is a node, named by its label
        names = list(args.tree_record.labels)
    names = model_flags.class_names(args.error, args, num_class, names)
    n, entries = args.batch, len(pool.entries)
    grids = []
    rows = []
    darknet = args.protocol == "darknet"
    for start in range(0, entries, n):
        images, valid = pool.batch(args.size, start, letterbox=not args.stretch, fill=args.fill, protocol=args.protocol)
        grid_out = None
        if args.keep_grids:
            grid_out = torch.empty((n, detector.S, detector.S, detector.B, 5 + num_class), dtype=torch.float32,
                                   device="cuda")
            grids.append(grid_out)
        if darknet and detector.wide is not None:
            det, score, count = detector.detect_tree_batch(images, pool.table, pool.eval_index, args.thresh, args.nms,
                                                           args.max_out, grid_out=grid_out, letterbox=True,
                                                           protocol="darknet")
            det, score, count = det.cpu().numpy(), score.cpu().numpy(), count.cpu().numpy()
            for k in range(valid):
                m = count[k]
                corners = det[k, :m, :4].copy().view("float32")             # words 0..3: the float corners' bit patterns
                for d, b, s in zip(det[k, :m], corners, score[k, :m]):
                    rows.append((pool.paths[start + k], names[d[4]], float(s)) + tuple(float(v) for v in b))
            continue
        if darknet:
            det, score, count = detector.detect_classes_batch(images, pool.table, pool.eval_index, args.thresh, args.nms,
                                                              args.max_out, grid_out=grid_out, letterbox=True,
                                                              protocol="darknet")
            det, score, count = det.cpu().numpy(), score.cpu().numpy(), count.cpu().numpy()
            for k in range(valid):
                for c in range(num_class):
                    m = count[k, c]
                    corners = det[k, c, :m, :4].copy().view("float32")      # words 0..3: the float corners' bit patterns
                    for b, s in zip(corners, score[k, c, :m]):
                        rows.append((pool.paths[start + k], names[c], float(s)) + tuple(float(v) for v in b))
            continue
        det, score, count = detector.detect_batch(images, pool.table, pool.eval_index, args.thresh, args.nms,
                                                  args.max_out, grid_out=grid_out, letterbox=not args.stretch)
        det, score, count = det.cpu().numpy(), score.cpu().numpy(), count.cpu().numpy()
        for k in range(valid):
            for d, s in zip(det[k, :count[k]], score[k, :count[k]]):
                rows.append((pool.paths[start + k], names[d[4]], float(s), int(d[0]), int(d[1]), int(d[2]), int(d[3])))
    lines = [("%s %s %f %f %f %f %f" if darknet else "%s %s %.6f %d %d %d %d") % r for r in rows]
    for line in lines:
        print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(line + "\n" for line in lines))
    result = {"rows": rows, "restored": restored, "detector": detector, "pool": pool, "topology": detector.topology}
    if args.keep_grids:
        result["grids"] = torch.cat(grids)[:entries]
    return result


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
