"""Darknet's `detector` command over Darknet's own files (not in the reference): a .data file names the data set
(utils/darknet_data.py), a .cfg file the model (utils/darknet_cfg.py), a .weights file its values.
    python -m tensorflow_yolo2_amd.darknet.detector train   <data> <cfg> [weights] [--iters N] [--region-stats] [solver flags]
    python -m tensorflow_yolo2_amd.darknet.detector valid   <data> <cfg> <weights>
    python -m tensorflow_yolo2_amd.darknet.detector map     <data> <cfg> <weights> [--metric 07|10]
    python -m tensorflow_yolo2_amd.darknet.detector anchors <data> --num K --size S

train    pascal_train_yolov2's trainer (its main, through the data-set seam) over the train= list: the cfg's recipe through
         apply_cfg, with the draw on (--draw-boxes: a crowded image trains a subset drawn anew at every use).  backup= is
         the snapshot directory: a run resumes from the latest train_iter_<i>.weights there.  [weights] is taken as the
         whole model where its float count is the cfg's, else as a backbone (net_utils.load_darknet_prefix, which refuses
         what it cannot place).  Every other flag of pascal_train_yolov2 passes through.
valid    detections over the valid= list under --protocol darknet; no label file is read.  eval=voc: one
         comp4_det_test_<class>.txt per class under results= (default "results"); eval=coco: the JSON of
         coco_eval.write_results, results=/coco_results.json, the image id from the digits of the file name
         (darknet_data.image_id_of) and the category id from darknet_data.coco_category_ids.
map      VOC AP per class and its mean over the valid= list's own label files: pascal_eval_yolov2.main through its seam,
         evaluate_yolov2 unchanged, IoU 0.5, --metric 07 (11-point, default) or 10 (area).
anchors  utils/anchors.kmeans_anchors over box_table_wh of the train= list at --size, printed as a cfg `anchors=` line with
         its mean_shape_iou.  Host only.

classes= of the .data file, the cfg's classes, the node count of the cfg's softmax_tree (a word tree: the label files'
classes are node indices) and the line count of names= must agree: a disagreement is an argument error that names the two
files.  --tree FILE and --hier-thresh X behind the positionals beat the cfg's softmax_tree and tree_thresh in train, valid
and map.  One process, one GPU."""
import argparse
import os
import sys

import numpy as np

PROG = "python -m tensorflow_yolo2_amd.darknet.detector"


def _split(argv):
    ap = argparse.ArgumentParser(prog=PROG, description="Darknet's detector command: train, valid, map, anchors")
    ap.add_argument("command", choices=("train", "valid", "map", "anchors"))
    ap.add_argument("data", help="a Darknet .data file")
    args, rest = ap.parse_known_args(argv)
    return ap, args, rest


def read_data_set(error, data_path, cfg_path=None, need=()):
    """(the .data record, the class names, the cfg record or None); the refusals are argument errors"""
    from ..utils import darknet_cfg, darknet_data
    try:
        data = darknet_data.read_data(data_path)
    except (OSError, ValueError) as e:
        error("%s" % e)
    for key in need:
        if getattr(data, key) is None:
            error("%s names no %s=" % (data_path, key))
    names = tuple(str(c) for c in range(data.classes))
    if data.names is not None:
        try:
            names = tuple(darknet_cfg.read_names(data.names))
        except OSError as e:
            error("%s: names=%s: %s" % (data_path, data.names, e))
        if len(names) != data.classes:
            error("%s has classes=%d, its names= file %s holds %d names" % (data_path, data.classes, data.names, len(names)))
    rec = None
    if cfg_path is not None:
        try:
            rec = darknet_cfg.load_graph(cfg_path)[0]       # a wide last layer (YOLO9000's) included: every command takes it
        except (OSError, ValueError) as e:
            error("%s" % e)
        if rec.classes != data.classes:
            error("%s has classes=%d, %s has classes=%d" % (data_path, data.classes, cfg_path, rec.classes))
        if rec.tree is not None:               # a word tree: the data set's classes are its nodes
            from ..yolo2_nets import yolov2
            try:
                tree = yolov2.load_cfg_tree(rec)
            except (OSError, ValueError) as e:
                error("%s" % e)
            if tree.n != data.classes:
                error("%s has classes=%d, the word tree %s of %s holds %d nodes" % (data_path, data.classes, tree.path,
                                                                                  cfg_path, tree.n))
    return data, names, rec


def _model_args(ap, rest, optional_weights):
    """the positionals behind <data>: <cfg> and [weights] / <weights>, the rest passes through"""
    if not rest or rest[0].startswith("-"):
        ap.error("a .cfg file is needed behind the .data file")
    cfg, rest = rest[0], rest[1:]
    weights = None
    if rest and not rest[0].startswith("-"):
        weights, rest = rest[0], rest[1:]
    elif not optional_weights:
        ap.error("a .weights file is needed behind the .cfg file")
    return cfg, weights, rest


def train(ap, data_path, rest):
    from ..pascal import pascal_train_yolov2 as T
    from ..utils import darknet_weights
    cfg, weights, rest = _model_args(ap, rest, True)
    data, names, rec = read_data_set(ap.error, data_path, cfg, need=("train",))
    argv = ["--cfg", cfg]
    if data.backup is not None:
        argv += ["--ckpt-dir", data.backup]
    if weights is not None:
        try:
            floats = darknet_weights.read(weights)[4].size
        except (OSError, ValueError) as e:
            ap.error("%s: %s" % (weights, e))
        argv += ["--darknet-weights" if floats == rec.floats else "--darknet-backbone", weights]
    args = T.parse_args(argv + rest, need_devkit=False, prog=PROG + " train <data> <cfg> [weights]", draw_boxes=True)
    args.dataset_name = data.train

    def dataset(a):
        from ..img_dataset.device_boxes import DeviceDarknet
        try:
            return DeviceDarknet(data.train, data.classes, names, batch_size=a.batch, flipped=a.flipped, seed=a.seed,
                                 augment=a.augmentation, max_boxes=a.max_boxes if a.box_labels else None, draw=a.draw_boxes)
        except (OSError, ValueError) as e:
            a.error("%s: train=%s: %s" % (data_path, data.train, e))
    return T.main(args, dataset=dataset)


def _eval_args(ap, data_path, rest, what, need):
    from ..pascal import pascal_eval_yolov2 as E
    cfg, weights, rest = _model_args(ap, rest, False)
    data, names, rec = read_data_set(ap.error, data_path, cfg, need=need)
    args = E.parse_args(["--cfg", cfg, "--darknet-weights", weights, "--protocol", "darknet"] + rest, need_devkit=False,
                        prog=PROG + " %s <data> <cfg> <weights>" % what)
    args.dataset_name = data.valid
    return E, data, names, args


def _valid_pool(data_path, data, names, args, labels):
    from ..img_dataset.device_boxes import DeviceDarknet
    try:
        return DeviceDarknet(data.valid, data.classes, names, batch_size=args.batch, labels=labels)
    except (OSError, ValueError) as e:
        args.error("%s: valid=%s: %s" % (data_path, data.valid, e))


def valid(ap, data_path, rest):
    from ..pascal import yolov2_model_flags as model_flags
    from ..utils import coco_eval, darknet_data, voc_eval
    E, data, names, args = _eval_args(ap, data_path, rest, "valid", ("valid",))
    imdb = _valid_pool(data_path, data, names, args, labels=False)
    snapshot, anchors, num_class, bn_eps = model_flags.find_snapshot(args, imdb.num_class)
    detector, _restored = model_flags.build_detector(args, snapshot, anchors, num_class, bn_eps)
    result = E.evaluate_yolov2(detector, imdb, args.size, args.thresh, args.nms, args.max_out, True, False, True,
                               args.max_per_class, True, args.fill, protocol="darknet")
    rows = result["rows"]
    directory = data.results if data.results is not None else "results"
    if data.eval == "coco":
        os.makedirs(directory, exist_ok=True)
        try:
            images = [{"id": darknet_data.image_id_of(e['imname'])} for e in imdb.entries]
        except ValueError as e:
            args.error("%s: eval=coco: %s" % (data_path, e))
        box = np.ascontiguousarray(rows["box"], np.float32).reshape(-1, 4)
        rows = dict(rows, bbox=coco_eval.row_xywh(box.view(np.int32), 1))
        dataset = {"images": images, "categories": darknet_data.coco_category_ids(data.classes)}
        files = [coco_eval.write_results(os.path.join(directory, "coco_results.json"), rows, dataset)]
    else:
        files = voc_eval.write_results_files(directory, "test", imdb.image_index, names, rows)
    print('{:d} images, {:d} detections, {:d} results file(s) under {:s}'.format(
        len(imdb.entries), len(rows["score"]), len(files), directory))
    result.update(results_files=files, detector=detector, imdb=imdb)
    return result


def mean_ap(ap, data_path, rest):
    E, data, names, args = _eval_args(ap, data_path, rest, "map", ("valid",))
    return E.main(args, dataset=lambda a: _valid_pool(data_path, data, names, a, labels=True))


def anchors(ap, data_path, rest):
    from ..img_dataset.device_boxes import build_tables
    from ..utils import anchors as A
    from ..utils import darknet_data
    sub = argparse.ArgumentParser(prog=PROG + " anchors <data>")
    sub.add_argument("--num", type=int, required=True, help="number of anchors")
    sub.add_argument("--size", type=int, required=True, help="input size the anchors are in cells (of stride 32) of")
    sub.add_argument("--seed", type=int, default=0)
    a = sub.parse_args(rest)
    if a.num < 1 or a.size < 32 or a.size % 32:
        sub.error("--num must be at least 1, --size a positive multiple of 32")
    data, _names, _rec = read_data_set(sub.error, data_path, need=("train",))
    try:
        entries = darknet_data.image_entries(data.train, data.classes)
        if not entries:
            raise ValueError("no image")
        table, boxes, counts = build_tables(entries, [0] * len(entries), [0] * len(entries), False)
        wh = A.box_table_wh(boxes, counts, table, a.size)
        found = A.kmeans_anchors(wh, k=a.num, seed=a.seed)
    except (OSError, ValueError) as e:
        sub.error("%s: train=%s: %s" % (data_path, data.train, e))
    iou = A.mean_shape_iou(wh, found)
    print("anchors = " + ",  ".join("%.4f,%.4f" % (w, h) for (w, h) in found))
    print("mean_shape_iou = %.4f (%d boxes of %d images, size %d)" % (iou, len(wh), len(entries), a.size))
    return {"anchors": found, "mean_shape_iou": iou, "boxes": len(wh)}


COMMANDS = {"train": train, "valid": valid, "map": mean_ap, "anchors": anchors}


def main(argv=None):
    ap, args, rest = _split(sys.argv[1:] if argv is None else list(argv))
    return COMMANDS[args.command](ap, args.data, rest)


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
