"""VOC mAP of the YOLOv2 anchor detector over an image set (not in the reference, which has no evaluation code):
    python -m tensorflow_yolo2_amd.pascal.pascal_eval_yolov2 --devkit data/VOCdevkit --image-set test \
        [--weights FILE | --ckpt-dir DIR] [--size 416] [--batch 32] [--metric 07|10]
        [--per-class [--max-per-class 32]] [--letterbox [--fill 127]] [--protocol repo|darknet] [--results-dir DIR]
The shape is pascal_eval_darknet.py's.  The images come from the device-resident pool in list order; per batch, four
calls on one stream and nothing on the host:
    DeviceVOC.eval_batch (resize) -> YOLOv2Detector.detect_batch = forward on the uint8 batch (moving statistics) ->
    y2_detect_anchor_batch (anchor decode, class choice, boxes in the pixels of each original image, class-aware NMS:
    one launch from the raw head) -> y2_voc_match_batch (TP / FP / ignored against the image's ground truth)
The det / score / count / flags of every batch land in ONE device buffer; after the last batch it is copied to the host
once and utils/detect_batch.map_from_flags makes the per-class curves and the APs.  A detection is an anchor's box with
its best class (score = objectness * class probability): one row per anchor.  With --per-class it is a row per class
whose score passes, as Darknet's `valid` writes (y2_detect_anchor_classes_batch; the matcher then runs over the
(image, class) segments): the protocol of the published YOLOv2 figures, up to this repository's integer-pixel IoU.
With --letterbox every image keeps its aspect ratio, as at Darknet's test time: eval_batch embeds it in a square of
--fill (y2_letterbox_u8_batch) and the detect launch un-maps the boxes from that rectangle (y2_detect_anchor_batch_lb,
y2_detect_anchor_classes_batch_lb); the default is the plain stretch, bit for bit as before.
The anchors and the class count are the snapshot's (pascal_train_yolov2.py); with neither --weights nor --ckpt-dir the
initial values are evaluated with the published VOC anchors: a plumbing run.  --darknet-weights FILE evaluates a file
Darknet wrote for yolov2-voc.cfg instead (the "darknet" topology of yolo2_nets/yolov2.py, net_utils.load_darknet_weights):
    pascal_eval_yolov2 --devkit data/VOCdevkit --darknet-weights yolov2-voc.weights --per-class --letterbox
or one it wrote for tiny-yolo-voc.cfg (the "tiny" topology, with its own published anchors): the file's float count says
which of the two graphs is built (net_utils.darknet_file_topology):
    pascal_eval_yolov2 --devkit data/VOCdevkit --darknet-weights tiny-yolo-voc.weights --protocol darknet
and --protocol darknet scores it as Darknet's `valid` would (it implies the two switches): the float letterbox with bars
of 0.5 in one launch from the pool (y2_letterbox_darknet_batch), Darknet's float un-map, float NMS and float corners
(y2_detect_anchor_classes_batch_dk), the matcher on those (y2_voc_match_batch_f), and "%f" results files:
    pascal_eval_yolov2 --devkit data/VOCdevkit --darknet-weights yolov2-voc.weights --protocol darknet
--cfg FILE names the Darknet cfg that goes with --darknet-weights: graph, class count, anchors and widths are the file's
(YOLOv2Detector.from_cfg); its class count must be the devkit's, since the evaluation stays VOC's.  --names FILE names
the classes of the --results-dir files.  --tree FILE (or softmax_tree= of --cfg) scores a word-tree model: every row's
only class is the node where the walk down the tree stops at --hier-thresh (tree_thresh of --cfg, else 0.5;
engine.word_tree_head), its score the objectness, and a detection matches a truth by equal node.

main(argv, dataset=None) takes the data set through a seam: `dataset(args)` returns the pool -- a DeviceBoxes
(img_dataset/device_boxes.py) with its `classes` and `image_index` -- where --devkit's DeviceVOC is not the one wanted
(darknet/detector.py: the valid= list of a .data file); with it --devkit is not required."""
import argparse
import sys

import numpy as np
import torch

from .. import engine
from ..utils import detect_batch
from . import yolov2_model_flags as model_flags


def parse_args(argv=None, need_devkit=True, prog=None):
    ap = argparse.ArgumentParser(prog=prog)
    ap.add_argument("--devkit", required=need_devkit, default=None, help="VOCdevkit directory (cfg.PASCAL_PATH)")
    ap.add_argument("--image-set", default="test")
    model_flags.add_model_flags(ap, 32, None, "evaluated", "the image set's class count")
    ap.add_argument("--thresh", type=float, default=0.005, help="score above which a box is a detection")
    ap.add_argument("--nms", type=float, default=0.45, help="IoU above which a box of the same class is suppressed")
    ap.add_argument("--max-out", type=int, default=100, help="detections kept per image")
    ap.add_argument("--per-class", action="store_true",
                    help="one row per (box, class) whose score passes, NMS per class: the rows Darknet's `valid` writes "
                         "and the published mAP figures are scored on (default: one row per box, its best class)")
    ap.add_argument("--max-per-class", type=int, default=32,
                    help="with --per-class: rows kept per image and class (Darknet has no cap: the count of saturated "
                         "segments is printed).  The device buffer takes 32 bytes per row, images x classes x this "
                         "many rows: about 100 MB for VOC07 test at the default")
    ap.add_argument("--letterbox", action="store_true",
                    help="keep every image's aspect ratio: embed it in the square input between bars of --fill and "
                         "un-map the boxes from that rectangle, as Darknet's test-time input (default: a plain stretch)")
    ap.add_argument("--fill", type=int, default=None, help="with --letterbox: the value of the bars, 0..255 (127)")
    ap.add_argument("--protocol", default="repo", choices=("repo", "darknet"),
                    help="darknet: Darknet's test-time protocol -- its float letterbox with bars of 0.5, its float un-map "
                         "and NMS, float corners in the rows and the results files.  Implies --per-class --letterbox; needs "
                         "--darknet-weights; not with --fill (default: this repository's integer-pixel protocol)")
    ap.add_argument("--results-dir", default=None,
                    help="write the devkit's comp4_det_<image-set>_<class>.txt files (image_id score xmin ymin xmax "
                         "ymax) there, from the rows of either form")
    ap.add_argument("--metric", default="07", choices=("07", "10"), help="07: 11-point AP; 10: area under the envelope")
    model_flags.add_test_flags(ap)
    args = ap.parse_args(argv)
    args.error = ap.error
    model_flags.resolve_cfg(ap, args, wide_head=True)
    model_flags.check_size(ap, args)
    if args.batch < 1 or args.max_out < 1 or args.width_div < 1 or args.max_per_class < 1:
        ap.error("--batch, --max-out, --max-per-class and --width-div must be at least 1")
    if args.protocol == "darknet":
        if args.fill is not None:
            ap.error("--fill is not read with --protocol darknet: Darknet's bars are 0.5")
        if not (args.darknet_weights or args.cfg):
            ap.error("--protocol darknet needs the darknet topology (--darknet-weights FILE): the paper topology's input "
                     "is BGR in [-1, 1)")
        args.per_class = args.letterbox = True
    if args.fill is None:
        args.fill = 127
    if not 0 <= args.fill <= 255:
        ap.error("--fill %d outside 0..255" % args.fill)
    model_flags.check_weights(ap, args)
    return args


def voc_dataset(args):
    """--devkit's pool"""
    from ..img_dataset.device_voc import DeviceVOC
    return DeviceVOC(args.image_set, batch_size=args.batch, devkit_path=args.devkit, flipped=False)


def main(argv=None, dataset=None):
    """argv: the command line, or an args record a caller parsed (parse_args) and filled; dataset: see above"""
    args = argv if isinstance(argv, argparse.Namespace) else parse_args(argv)
    imdb = (dataset or voc_dataset)(args)
    snapshot, anchors, num_class, bn_eps = model_flags.find_snapshot(args, imdb.num_class)
    if args.cfg_record is not None and num_class != imdb.num_class:     # the evaluation is VOC's
        args.error("--cfg %s has classes=%d, the image set %s has %d classes" %
                   (args.cfg, num_class, getattr(args, "dataset_name", args.image_set), imdb.num_class))
    names = model_flags.class_names(args.error, args, num_class, imdb.classes[:num_class])
    if num_class != imdb.num_class:
        raise ValueError("snapshot %s: num_class is %d, the image set has %d" % (snapshot, num_class, imdb.num_class))
    detector, restored = model_flags.build_detector(args, snapshot, anchors, num_class, bn_eps)
    result = evaluate_yolov2(detector, imdb, args.size, args.thresh, args.nms, args.max_out, args.metric == "07",
                             args.keep_grids, args.per_class, args.max_per_class, args.letterbox, args.fill,
                             protocol=args.protocol)
    for c in sorted(result["aps"]):
        print('AP for {:s} = {:.4f}'.format(imdb.classes[c], result["aps"][c]))
    print('Mean AP = {:.4f} ({:d} images, {:d} detections, VOC{:s} metric)'.format(
        result["mAP"], len(imdb.entries), len(result["rows"]["flag"]), "07" if args.metric == "07" else "10+"))
    if args.per_class and result["tree_rows"]:
        print('{:d} of {:d} images reached --max-out {:d}'.format(result["saturated"], result["count"].size, args.max_out))
    elif args.per_class:
        print('{:d} of {:d} (image, class) segments reached --max-per-class {:d}'.format(
            result["saturated"], result["count"].size, args.max_per_class))
    if args.results_dir:
        from ..utils import voc_eval
        result["results_files"] = voc_eval.write_results_files(args.results_dir, args.image_set, imdb.image_index,
                                                               names, result["rows"])
    result.update(restored=restored, detector=detector, imdb=imdb, topology=detector.topology)
    return result


def evaluate_yolov2(detector, imdb, size, thresh=0.005, nms=0.45, max_out=100, use_07_metric=True, keep_grids=False,
                    per_class=False, max_per_class=32, letterbox=False, fill=127, protocol="repo", tree_rows=None):
    """one pass over imdb's image list through `detector` (a YOLOv2Detector of imdb.batch_size images of `size`):
    {"mAP", "aps", "rows", "count", "npos"[, "grids"]} as pascal_eval_darknet.evaluate; everything per image runs on the
    device, one copy at the end.  per_class: one row per (candidate, class) as Darknet's `valid` writes them, at most
    max_per_class per image and class (max_out is not read); an image is then num_class segments of the same buffer,
    "count" is [entries][num_class] and "saturated" the number of segments whose count reached max_per_class.
    letterbox: the batches are letterboxed between bars of `fill` and the boxes un-mapped from each picture's rectangle.
    protocol="darknet": Darknet's test-time protocol -- its float letterbox from the pool to the network's input in one
    launch, its float un-map and NMS, the matcher on float corners (csrc/darknet_io.hip).  It is per_class and
    letterboxed by definition (both must be set), needs a detector of the "darknet" topology and the default `fill`;
    rows["box"] is then float32.
    tree_rows (None: the detector has a wide head): with per_class or protocol="darknet", the rows come from
    detector.detect_tree_batch instead -- on a word tree a candidate has ONE class, its node, so an image is one segment of
    max_out rows (max_per_class is not read), matched on the image's own index; "count" is [entries] and "saturated" the
    number of images whose count reached max_out.  It needs a detector with a tree.  Narrow tree models keep the
    per-class segments unless it is set; without per_class and protocol="darknet" it changes nothing (detect_batch's rows
    are already these)"""
    tree_rows = getattr(detector, "wide", None) is not None if tree_rows is None else bool(tree_rows)
    if tree_rows and getattr(detector, "tree", None) is None:
        raise ValueError("tree_rows=True needs a detector with a word tree: the rows' class is the tree's node")
    if protocol not in ("repo", "darknet"):
        raise ValueError("protocol %r is neither 'repo' nor 'darknet'" % (protocol,))
    darknet = protocol == "darknet"
    if darknet and not (per_class and letterbox):
        raise ValueError("protocol='darknet' scores one row per (box, class) on a letterboxed input: per_class=True, "
                         "letterbox=True")
    if darknet and getattr(detector, "topology", "paper") not in ("darknet", "tiny"):
        raise ValueError("protocol='darknet' needs a detector of the \"darknet\" topology, not %r"
                         % (getattr(detector, "topology", "paper"),))
    match = engine.voc_match_batch_f if darknet else engine.voc_match_batch
    n = imdb.batch_size
    assert detector.batch == n and detector.size == size, (detector.batch, detector.size, n, size)
    S, B, D = detector.S, detector.B, 5 + detector.num_class
    entries = len(imdb.entries)
    batches = (entries + n - 1) // n
    # a segment is what the matcher walks as one "image": the image, or with per_class one class of it
    tree_rows = tree_rows and (per_class or darknet)
    segs, R = (detector.num_class, max_per_class) if per_class and not tree_rows else (1, max_out)
    N = batches * n * segs
    # det [N][R][6] | score [N][R] (float bits) | flags [N][R] | count [N]: one buffer, one copy
    words = N * R * 8 + N
    acc = torch.empty(words, dtype=torch.int32, device="cuda")
    det = acc[:N * R * 6].view(N, R, 6)
    score = acc[N * R * 6:N * R * 7].view(torch.float32).view(N, R)
    flags = acc[N * R * 7:N * R * 8].view(N, R)
    count = acc[N * R * 8:]
    grids = torch.empty((batches * n, S, S, B, D), dtype=torch.float32, device="cuda") if keep_grids else None
    seg_index = torch.empty(n * segs, dtype=torch.int32, device="cuda") if segs > 1 else None
    difficult = imdb.difficult
    for k in range(batches):
        lo, m = k * n * segs, n * segs
        if darknet:
            images, _valid = imdb.eval_batch(size, k * n, letterbox=True, fill=fill, protocol="darknet")
        else:
            images, _valid = imdb.eval_batch(size, k * n, letterbox=letterbox, fill=fill)
        out = (det[lo:lo + m], score[lo:lo + m], count[lo:lo + m])
        grid_out = grids[k * n:k * n + n] if grids is not None else None
        index = imdb.eval_index
        if tree_rows:                                                        # one segment per image: its own index
            detector.detect_tree_batch(images, imdb.table, index, thresh, nms, max_out, out=out, grid_out=grid_out,
                                       letterbox=letterbox, protocol=protocol)
        elif per_class:                                                      # (protocol="darknet" is per_class, letterboxed)
            detector.detect_classes_batch(images, imdb.table, index, thresh, nms, max_per_class, out=out,
                                          grid_out=grid_out, letterbox=letterbox, protocol=protocol)
            seg_index.view(n, segs).copy_(index[:n, None].expand(n, segs))   # on the device: nothing waits
            index = seg_index
        else:
            detector.detect_batch(images, imdb.table, index, thresh, nms, max_out, out=out, grid_out=grid_out,
                                  letterbox=letterbox)
        match(det[lo:lo + m], score[lo:lo + m], count[lo:lo + m], imdb.boxes, imdb.counts, difficult, index, 0.5,
              out=flags[lo:lo + m])
    host = acc.cpu().numpy()                                  # the one device-to-host copy (it waits for the stream)
    live_segs = entries * segs
    det_h = host[:N * R * 6].reshape(N, R, 6)[:live_segs]
    score_h = host[N * R * 6:N * R * 7].view(np.float32).reshape(N, R)[:live_segs]
    flags_h = host[N * R * 7:N * R * 8].reshape(N, R)[:live_segs]
    count_h = host[N * R * 8:][:live_segs]
    live = np.arange(R)[None, :] < count_h[:, None]            # image order (then class), each segment in descending score
    box = det_h[live][:, :4]
    if darknet:
        box = np.ascontiguousarray(box).view(np.float32)       # words 0..3 hold the bit patterns of the float corners
    rows = {"image": np.nonzero(live)[0] // segs, "box": box, "class": det_h[live][:, 4],
            "candidate": det_h[live][:, 5], "score": score_h[live], "flag": flags_h[live]}
    npos = detect_batch.npos_from_objects([o[4] for e in imdb.entries for o in e['objs']],
                                          [d for e in imdb.entries for d in e['difficult']])
    mAP, aps = detect_batch.map_from_flags((rows["class"], rows["score"], rows["flag"]), npos,
                                           use_07_metric=use_07_metric)
    result = {"mAP": mAP, "aps": aps, "rows": rows, "count": count_h.copy(), "npos": npos}
    result["tree_rows"] = tree_rows
    if per_class:
        result["count"] = result["count"].reshape(entries, segs) if not tree_rows else result["count"]
        result["saturated"] = int((count_h >= R).sum())
    if grids is not None:
        result["grids"] = grids[:entries]
    return result


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
