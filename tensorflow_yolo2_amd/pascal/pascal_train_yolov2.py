"""Train the YOLOv2 anchor detector (yolo2_nets/yolov2.py; not in the reference, whose trainer is the grid model) on VOC:
    python -m tensorflow_yolo2_amd.pascal.pascal_train_yolov2 --devkit data/VOCdevkit --iters 20 \
        [--multi-scale] [--augment] [--anchors voc|kmeans] [--ckpt-dir DIR] [--imagenet-ckpt-dir DIR | --darknet-backbone FILE]
        [--topology paper|darknet] [--darknet-weights FILE] [--cfg FILE [--single-scale]] [--region-stats]
        [--box-labels [--max-boxes 30] [--area-weight] [--prior-images 12800] [--draw-boxes]]
        [--solver darknet [--lr .001] [--momentum .9] [--decay .0005] [--burn-in 1000] [--power 4]
                          [--policy steps --steps 40000,60000 --scales .1,.1 | --policy poly --max-batches N | --policy constant]]
The flags are pascal_train_darknet.py's where they apply.  The batches always come from the device-resident pool
(img_dataset.device_voc.DeviceVOC.get(size)): the uint8 batch goes straight into YOLOv2Trainer.step, whose first layer
converts it, and the label grid [N,S,S,5+C] (one box per cell) is the anchor loss's input as it stands.  --multi-scale
redraws the size of iteration i from --ms-sizes every --ms-period iterations (trainer.multi_scale_size); --augment is
Darknet's crop / mirror / HSV recipe in the device kernels.

--box-labels trains on the box list instead (get(size) with max_boxes: truth [N,T,5] + ntruth [N], EVERY object of an
image, so two objects of one cell both reach their anchors; engine.yolov2_loss_boxes).  With it, --area-weight is
Darknet's (2 - w h) weight of the coord terms and --prior-images the number of images (12800 in Darknet) during which
every prediction without an object is pulled toward its anchor.  The list encoder draws no random numbers, so a resumed
run moves the data and augmentation streams exactly as without it; the prior's switch reads the snapshot's iteration.
--draw-boxes (off by default) is Darknet's shuffle-then-cut: an image whose window keeps more than --max-boxes objects
trains a subset drawn anew every time, not the first ones (augment.encode_box_list_draw; y2_encode_box_list_draw).  Its
keys come from a stream of their own, one per sample, which a resumed run moves with the other two.

main(argv, dataset=None) takes the data set through a seam: `dataset(args)` returns the pool -- a DeviceBoxes
(img_dataset/device_boxes.py) -- where --devkit's DeviceVOC is not the one wanted, as darknet/detector.py and
coco/coco_train_yolov2.py do; with it --devkit is not required.

--solver darknet replaces Adam by Darknet's solver (utils/solver.py; engine.DarknetSGD): momentum SGD, weight decay on
the convolution filters only, and the rate schedule -- a burn-in lr (t / burn_in)^power, then the policy.  The defaults
are yolov2-voc.cfg's; the losses here are batch means, so --lr times the mean gradient is Darknet's learning_rate /
batch times its summed gradient: the cfg's learning_rate is the value to give.  The schedule counts APPLIED steps on the device (a step skipped by the overflow guard does not move it); the
rate the 10-iteration line prints is the host's current_rate of the iteration number.

Snapshots are `train_iter_<i>.npz` (net_utils.save_yolov2_variables: the three stacks, the anchors, the three Adam
states -- or the three Momentum slots and the solver record -- with their one loss scaler); a run with --ckpt-dir resumes from the latest, moves the data order and the
augmentation stream to where the saved run stood, and so continues it.  Without a snapshot, --imagenet-ckpt-dir takes
the Darknet-19 backbone from the latest classifier snapshot there, and --darknet-backbone FILE from a file Darknet wrote
(darknet19_448.conv.23; net_utils.read_darknet_backbone): the trainer then runs batch-norm epsilon 1e-6, which its
snapshots record (yolov2/bn_eps) and a resumed run takes from them.  --anchors kmeans clusters the image set's boxes
(utils/anchors.py) instead of using the published VOC anchors; a resumed run keeps its snapshot's anchors.

--topology darknet trains the graph of yolov2-voc.cfg instead (yolov2.YOLOv2DarknetTrainer): --darknet-weights FILE starts
from a whole Darknet file (it implies the topology), --darknet-backbone FILE from the leading layers of a shorter one
(net_utils.load_darknet_prefix: no first-layer fold, this graph takes Darknet's input).  Its snapshots are
`train_iter_<i>.weights`, written by net_utils.save_darknet_weights with seen = i * batch, which Darknet and
pascal_eval_yolov2 --darknet-weights read; a run with --ckpt-dir resumes from the latest at iteration seen // batch and
moves the data as above.  A .weights file carries no optimizer state and no anchors: the moments and the loss scale start
afresh, as in Darknet, and the anchors are the flags'.  A --ckpt-dir that holds the other topology's snapshots is an error.

--topology tiny trains the graph of tiny-yolo-voc.cfg with the same trainer, files, snapshots and resume, and that graph's
published anchors.  --darknet-weights FILE chooses between the two Darknet graphs by the file's float count
(net_utils.darknet_file_topology); a stated --topology that contradicts the file is an argument error, and a --ckpt-dir
whose .weights files belong to the other Darknet graph fails in the loader, by the float count.

--cfg FILE trains the graph a Darknet cfg describes (utils/darknet_cfg.py; yolov2.YOLOv2DarknetTrainer.from_cfg): the file
decides the topology, the class count, the anchors and the widths -- the float count of --darknet-weights is checked against
it, not guessed from -- and implies Darknet's recipe: --augment --box-labels --area-weight --prior-images 12800 --solver
darknet, --multi-scale where the file says random=1 (--single-scale keeps one size), and the file's jitter, hue, saturation,
exposure, solver values, width (--size) and batch (--batch).  A flag given on the command line beats the file; the resolved
recipe is printed once.  It goes with --darknet-weights, --darknet-backbone or a fresh model, and with a --ckpt-dir of
.weights snapshots; not with --topology paper, --imagenet-ckpt-dir, --anchors or a --ckpt-dir of .npz snapshots.  The image
set's class count must be the file's.  A file whose last convolution is wider than a stack's row (YOLO9000's 28,269
filters) loads under wide_head=True by itself (darknet_cfg.load_graph; `map=` stays unread): that layer trains as
engine.WideHead under --dtype f16, and the train_iter_<i>.weights snapshots hold it as the file's last layer.

--region-stats (with --box-labels or --cfg) prints Darknet's region-layer line for the last step beside the 10-iteration
line: `Region Avg IOU, Class, Obj, No Obj, Avg Recall, count`, computed on the device from the step's head output and its
box list (engine.yolov2_region_stats; utils/region_loss.py region_stats_boxes).

--tree FILE (or softmax_tree= of --cfg; the flag beats the file) trains a word tree (utils/word_tree.py): the classes are
the tree's nodes, a truth's class is a node index -- any node, an inner one too -- and the class loss is the softmax per
group of siblings along the truth's path to the root (engine.yolov2_loss_boxes_tree); --region-stats then prints the mean
abs[class] as Class (engine.yolov2_region_stats_tree).  It needs the box list (--box-labels or --cfg); --hier-thresh is
kept for the detector.

One process, one GPU."""
import argparse
import os

import numpy as np
import torch

from . import yolov2_model_flags as model_flags
from ..utils.timer import Timer
from ..yolo2_nets import net_utils, yolov2


def parse_args(argv=None, need_devkit=True, prog=None, draw_boxes=None):
    """need_devkit=False: a caller that brings its own data set (main's `dataset`); prog: its name in the usage line;
    draw_boxes: its default of --draw-boxes where the recipe has box labels (None: off)"""
    from ..trainer import MULTI_SCALE_SIZES
    ap = argparse.ArgumentParser(prog=prog)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=None, help="24, or the batch of --cfg")
    ap.add_argument("--size", type=int, default=None, help="416, or the width of --cfg")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--devkit", required=need_devkit, default=None, help="VOCdevkit directory (cfg.PASCAL_PATH)")
    ap.add_argument("--image-set", default="trainval")
    ap.add_argument("--flipped", action="store_true", help="cfg.FLIPPED: append horizontally flipped copies")
    ap.add_argument("--multi-scale", action="store_true", help="input size redrawn every --ms-period iterations")
    ap.add_argument("--ms-sizes", default=",".join(str(v) for v in MULTI_SCALE_SIZES), help="comma-separated sizes")
    ap.add_argument("--ms-period", type=int, default=10)
    ap.add_argument("--augment", action="store_true", help="random crop / pad window, mirror and HSV distortion")
    ap.add_argument("--jitter", type=float, default=None, help="window edges move by up to this share of the image (0.3)")
    ap.add_argument("--hue", type=float, default=None, help="hue shift drawn from [-hue, hue] turns (0.1)")
    ap.add_argument("--saturation", type=float, default=None, help="saturation factor drawn from [1 / s, s] (1.5)")
    ap.add_argument("--exposure", type=float, default=None, help="exposure factor drawn from [1 / e, e] (1.5)")
    ap.add_argument("--ckpt-dir", default=None, help="directory of train_iter_<i>.npz snapshots: resume from the latest")
    ap.add_argument("--save-every", type=int, default=40000)
    ap.add_argument("--imagenet-ckpt-dir", default=None, help="classifier snapshots to take the backbone from")
    ap.add_argument("--darknet-backbone", default=None,
                    help="a Darknet .weights file to take the Darknet-19 backbone from (darknet19_448.conv.23); the trainer "
                         "then runs Darknet's batch-norm epsilon 1e-6; not with --imagenet-ckpt-dir")
    ap.add_argument("--topology", default=None, choices=yolov2.TOPOLOGIES,
                    help="paper (default): the graph of yolo2_nets/yolov2.py, .npz snapshots; darknet: the graph of "
                         "yolov2-voc.cfg (YOLOv2DarknetTrainer), whose snapshots are train_iter_<i>.weights files Darknet "
                         "reads -- such a file carries no optimizer state, so a resumed run starts the moments and the loss "
                         "scale afresh, as Darknet does, and takes the iteration from the file's `seen` / --batch; tiny: "
                         "the graph of tiny-yolo-voc.cfg, the same trainer, snapshots and resume, its own published anchors")
    ap.add_argument("--darknet-weights", default=None,
                    help="start from a whole Darknet .weights file (yolov2-voc.weights or tiny-yolo-voc.weights); its float "
                         "count chooses --topology darknet or tiny, and a stated --topology that contradicts the file is "
                         "an error; not with --darknet-backbone or --imagenet-ckpt-dir")
    ap.add_argument("--cfg", default=None,
                    help="a Darknet .cfg file: it decides the topology, class count, anchors and widths and implies "
                         "Darknet's recipe (--augment --box-labels --area-weight --prior-images 12800 --solver darknet, "
                         "multi-scale on random=1, the file's jitter / hue / saturation / exposure / solver values / width "
                         "/ batch); a flag given on the command line beats the file.  Not with --topology paper, "
                         "--imagenet-ckpt-dir, --anchors or .npz snapshots")
    model_flags.add_tree_flags(ap)
    ap.add_argument("--single-scale", action="store_true", help="with --cfg: one input size even where random=1")
    ap.add_argument("--region-stats", action="store_true",
                    help="print Darknet's region-layer line (Avg IOU, Class, Obj, No Obj, Avg Recall, count) of the last "
                         "step every 10 iterations (needs --box-labels or --cfg)")
    ap.add_argument("--anchors", default=None, choices=("voc", "kmeans"),
                    help="voc: the published VOC anchors; kmeans: cluster the image set's boxes at --size")
    ap.add_argument("--box-labels", action="store_true", help="train on the box list (every object), not the label grid")
    ap.add_argument("--max-boxes", type=int, default=None, help="rows of the box list (default 30; needs --box-labels)")
    ap.add_argument("--area-weight", action="store_true", help="coord terms times 2 - w h (needs --box-labels)")
    ap.add_argument("--prior-images", type=int, default=None,
                    help="images during which un-owned predictions are pulled toward their anchors (needs --box-labels)")
    ap.add_argument("--draw-boxes", action="store_true",
                    help="an image with more than --max-boxes objects keeps a subset drawn anew at every use, Darknet's "
                         "shuffle-then-cut, not the first ones (needs --box-labels)")
    ap.add_argument("--solver", default="adam", choices=("adam", "darknet"),
                    help="adam: tf.train.AdamOptimizer defaults; darknet: momentum SGD + filter decay + rate schedule")
    ap.add_argument("--lr", type=float, default=None, help="base rate (0.001; needs --solver darknet, as all below)")
    ap.add_argument("--momentum", type=float, default=None, help="0.9")
    ap.add_argument("--decay", type=float, default=None, help="weight decay of the convolution filters (0.0005)")
    ap.add_argument("--burn-in", type=int, default=None, help="steps of the lr (t / burn_in)^power ramp (1000)")
    ap.add_argument("--power", type=int, default=None, help="exponent of the ramp and of the poly policy (4)")
    ap.add_argument("--policy", default=None, choices=("constant", "steps", "poly"), help="after the ramp (steps)")
    ap.add_argument("--steps", default=None, help="comma-separated steps of the steps policy (40000,60000)")
    ap.add_argument("--scales", default=None, help="comma-separated factors, one per step (.1,.1)")
    ap.add_argument("--max-batches", type=int, default=None, help="where the poly policy reaches zero")
    ap.add_argument("--width-div", type=int, default=1, help="divide every inner width (tests)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    args.error, args.topology_stated = ap.error, args.topology
    apply_cfg(ap, args)
    if args.size < 32 or args.size % 32:
        ap.error("--size %d: the detector head needs a positive multiple of 32 (S = size / 32)" % args.size)
    if args.batch < 1 or args.iters < 0 or args.save_every < 1 or args.width_div < 1:
        ap.error("--batch, --save-every and --width-div must be at least 1, --iters at least 0")
    if args.darknet_backbone and args.imagenet_ckpt_dir:
        ap.error("--darknet-backbone and --imagenet-ckpt-dir name two backbones: give one")
    if args.darknet_weights:
        if args.darknet_backbone or args.imagenet_ckpt_dir:
            ap.error("--darknet-weights holds the whole model: not with --darknet-backbone or --imagenet-ckpt-dir")
        if args.topology == "paper":
            ap.error("--darknet-weights is a file of the darknet topology: not with --topology paper")
        if args.topology is None:
            args.topology = "darknet"             # until main() has read the file's float count (file_topology)
    if args.topology is None:
        args.topology = "paper"
    if args.topology in yolov2.DARKNET_FILE_TOPOLOGIES and args.imagenet_ckpt_dir:
        ap.error("--imagenet-ckpt-dir feeds the paper topology; with --topology %s give --darknet-backbone FILE" %
                 args.topology)
    try:
        args.ms_sizes = tuple(int(v) for v in str(args.ms_sizes).split(",") if v.strip())
    except ValueError:
        ap.error("--ms-sizes %r is not a comma-separated list of integers" % (args.ms_sizes,))
    if args.multi_scale:
        bad = [v for v in args.ms_sizes if v < 32 or v % 32]
        if not args.ms_sizes or bad:
            ap.error("--ms-sizes: the detector head cannot take %s (positive multiples of 32 only)" % (bad or "an empty list"))
        if args.ms_period < 1:
            ap.error("--ms-period must be at least 1")
    if not args.box_labels and (args.area_weight or args.prior_images or args.max_boxes is not None):
        ap.error("--max-boxes, --area-weight and --prior-images need --box-labels")
    if args.draw_boxes and not args.box_labels:
        ap.error("--draw-boxes chooses among the objects of the box list: it needs --box-labels")
    if draw_boxes and args.box_labels:
        args.draw_boxes = True
    if args.prior_images is None:
        args.prior_images = 0
    if args.max_boxes is None:
        args.max_boxes = 30
    if not 1 <= args.max_boxes <= 1024 or args.prior_images < 0:
        ap.error("--max-boxes must lie in 1..1024, --prior-images must not be negative")
    given = [f for f in SOLVER_FLAGS if getattr(args, f) is not None]
    if args.solver != "darknet" and given:
        ap.error("%s need(s) --solver darknet" % ", ".join("--" + f.replace("_", "-") for f in given))
    args.solver_record = None
    if args.solver == "darknet":
        from ..utils.solver import Solver
        d = Solver()
        if args.cfg_record is not None:         # the file's values where no flag is given
            d = args.cfg_record.solver
            if args.policy == "poly" and args.max_batches is None:
                args.max_batches = args.cfg_record.max_batches
        try:
            steps = d.steps if args.steps is None else tuple(int(v) for v in args.steps.split(",") if v.strip())
            scales = d.scales if args.scales is None else tuple(float(v) for v in args.scales.split(",") if v.strip())
        except ValueError:
            ap.error("--steps takes comma-separated integers, --scales comma-separated numbers")
        if (args.steps is None) != (args.scales is None) and len(steps) != len(scales):
            ap.error("--steps %s and --scales %s: one scale per step" % (steps, scales))
        pick = lambda v, dv: dv if v is None else v
        try:
            args.solver_record = Solver(pick(args.lr, d.learning_rate), pick(args.momentum, d.momentum),
                                        pick(args.decay, d.decay), pick(args.policy, d.policy),
                                        pick(args.burn_in, d.burn_in), pick(args.power, d.power), steps, scales,
                                        pick(args.max_batches, d.max_batches))
        except ValueError as e:
            ap.error("--solver darknet: %s" % e)
    args.augmentation = None
    if args.augment:
        from ..img_dataset.augment import Augment
        try:
            args.augmentation = Augment(args.jitter, args.hue, args.saturation, args.exposure)
        except ValueError as e:
            ap.error("--augment: %s" % e)
    return args


def apply_cfg(ap, args):
    """--cfg: read the file (args.cfg_record; None without the flag), refuse what contradicts it, and fill every flag that
    was not given from it -- then today's defaults, with or without a file"""
    args.cfg_record = args.cfg_graph = None
    args.wide_head = False
    pick = lambda v, dv: dv if v is None else v
    if args.single_scale and not args.cfg:
        ap.error("--single-scale needs --cfg")
    if args.cfg:
        from ..utils import darknet_cfg
        if args.topology == "paper":
            ap.error("--cfg describes a Darknet graph: not with --topology paper")
        if args.imagenet_ckpt_dir:
            ap.error("--cfg describes a Darknet graph: --imagenet-ckpt-dir feeds the paper topology; give --darknet-backbone")
        if args.anchors is not None:
            ap.error("--cfg holds the anchors: not with --anchors")
        if args.width_div != 1:
            ap.error("--cfg holds the widths: not with --width-div")
        try:
            # a last layer wider than a stack's row (YOLO9000's) loads under wide_head=True and trains as engine.WideHead
            rec, args.cfg_graph, args.wide_head = darknet_cfg.load_graph(
                args.cfg, 1024 if args.dtype == "f32" else darknet_cfg.MAX_OUT_WIDTH)
            args.cfg_record = rec
        except (OSError, ValueError) as e:
            ap.error("--cfg: %s" % e)
        if args.wide_head and args.dtype != "f16":
            ap.error("--cfg %s has a wide head (%d filters), which trains under --dtype f16 only: not %s" %
                     (args.cfg, args.cfg_graph.file_layers[-1][2], args.dtype))
        found = {"chain": "tiny", "passthrough": "darknet"}[args.cfg_graph.shape]
        if args.topology not in (None, found):
            ap.error("--topology %s, but --cfg %s describes the %s graph" % (args.topology, args.cfg, found))
        args.topology = args.topology_stated = found
        args.augment = args.box_labels = args.area_weight = True
        args.solver = "darknet"
        if rec.random and not args.single_scale:
            args.multi_scale = True
        args.prior_images = pick(args.prior_images, yolov2.YOLOv2DarknetTrainer.CFG_PRIOR_IMAGES)
        args.size, args.batch = pick(args.size, rec.size), pick(args.batch, rec.batch)
        aug = rec.augmentation
        args.jitter, args.hue = pick(args.jitter, aug.jitter), pick(args.hue, aug.hue)
        args.saturation, args.exposure = pick(args.saturation, aug.saturation), pick(args.exposure, aug.exposure)
    args.size, args.batch = pick(args.size, 416), pick(args.batch, 24)
    args.jitter, args.hue = pick(args.jitter, 0.3), pick(args.hue, 0.1)
    args.saturation, args.exposure = pick(args.saturation, 1.5), pick(args.exposure, 1.5)
    args.anchors = pick(args.anchors, "voc")
    if args.region_stats and not args.box_labels:
        ap.error("--region-stats reads the box list: it needs --box-labels or --cfg")
    model_flags.resolve_tree(ap, args)
    if args.tree_record is not None and not args.box_labels:
        ap.error("a word tree trains on the box list (a truth's class is a node): it needs --box-labels or --cfg")


def print_recipe(args):
    """the recipe a --cfg run resolved to, once at start: the file's values and what a flag put in their place"""
    aug = args.augmentation
    print("cfg {:s}: topology {:s}, {:d} classes, {:d} anchors, size {:d}, batch {:d}, multi-scale {:s}".format(
        args.cfg, args.topology, args.cfg_record.classes, args.cfg_record.num, args.size, args.batch,
        "on" if args.multi_scale else "off"))
    print("cfg recipe: box labels, area weight, prior images {:d}, jitter {:g}, hue {:g}, saturation {:g}, exposure {:g}, "
          "scales {}".format(args.prior_images, aug.jitter, aug.hue, aug.saturation, aug.exposure,
                             ", ".join("%s %g" % kv for kv in args.cfg_record.scales)))
    print("cfg solver: {!r}".format(args.solver_record))


SOLVER_FLAGS = ("lr", "momentum", "decay", "burn_in", "power", "policy", "steps", "scales", "max_batches")


TRAINERS = {"paper": yolov2.YOLOv2Trainer, "darknet": yolov2.YOLOv2DarknetTrainer, "tiny": yolov2.YOLOv2DarknetTrainer}


def file_topology(args, num_class):
    """the topology of a run that starts from --darknet-weights: the graph whose float count the file has (at the image
    set's classes, five anchors and --width-div); a stated --topology that is another one is an argument error"""
    found = net_utils.darknet_file_topology(args.darknet_weights, num_class, len(yolov2.ANCHORS_VOC), args.width_div)
    if args.topology_stated not in (None, found):
        args.error("--topology %s, but --darknet-weights %s holds the %s graph" %
                   (args.topology_stated, args.darknet_weights, found))
    return found


def step_size(args, i):
    """input size of training iteration i (1-based, counted over resumed runs): a function of the flags alone"""
    if not args.multi_scale:
        return args.size
    from ..trainer import multi_scale_size
    return multi_scale_size(i, args.ms_sizes, args.ms_period)


def skip_batches(imdb, batches):
    """move a fresh pool to where it stands after `batches` calls of get(): the order's cursor and reshuffles, one
    augmentation row per sample (a row's draws do not depend on the output size) and, with the draw, one key"""
    for _ in range(batches * imdb.batch_size):
        imdb.next_sample()


def voc_dataset(args):
    """--devkit's pool"""
    from ..img_dataset.device_voc import DeviceVOC
    return DeviceVOC(args.image_set, batch_size=args.batch, devkit_path=args.devkit, flipped=args.flipped,
                     seed=args.seed, augment=args.augmentation, max_boxes=args.max_boxes if args.box_labels else None,
                     draw=args.draw_boxes)


def main(argv=None, dataset=None):
    """argv: the command line, or an args record a caller parsed (parse_args) and filled; dataset: see above"""
    args = argv if isinstance(argv, argparse.Namespace) else parse_args(argv)
    imdb = (dataset or voc_dataset)(args)
    latest = None
    rec = args.cfg_record
    if rec is not None:
        if imdb.num_class != rec.classes:
            args.error("--cfg %s has classes=%d, the image set %s has %d classes" %
                       (args.cfg, rec.classes, getattr(args, "dataset_name", args.image_set), imdb.num_class))
        print_recipe(args)
    model_flags.check_tree(args.error, args, imdb.num_class)
    if rec is None and args.darknet_weights:
        args.topology = file_topology(args, imdb.num_class)
    darknet = args.topology in yolov2.DARKNET_FILE_TOPOLOGIES
    if args.ckpt_dir:
        os.makedirs(args.ckpt_dir, exist_ok=True)
        try:
            latest = net_utils.latest_yolov2_snapshot(args.ckpt_dir, args.topology)
        except ValueError as e:
            if rec is None:
                raise
            args.error("--cfg: %s" % e)       # a directory of .npz snapshots
    if rec is not None:
        anchors = rec.anchors
    elif latest and not darknet:              # a .weights file carries no anchors: the flags'
        anchors = net_utils.read_yolov2_meta(latest)[0]
    elif args.anchors == "kmeans":
        from ..utils import anchors as A
        wh = A.box_table_wh(imdb.boxes, imdb.counts, imdb.table, args.size, entries=len(imdb.entries))
        anchors = A.kmeans_anchors(wh, k=len(yolov2.ANCHORS_VOC), seed=args.seed)
        # cell units at --size; the loss and the decode read anchors in cells of whatever size a step runs at
        print("k-means anchors at {:d} (mean shape IoU {:.4f}): {}".format(
            args.size, A.mean_shape_iou(wh, anchors), np.round(anchors, 4).tolist()))
    else:
        anchors = yolov2._TOPOLOGY[args.topology].anchors     # the graph's published ones
    first = step_size(args, 1) if args.multi_scale else args.size
    # Darknet's layers were trained with its batch-norm epsilon; a resumed run keeps its snapshot's (yolov2/bn_eps)
    bn_eps = yolov2.DARKNET_BN_EPS if args.darknet_backbone else None
    if latest and bn_eps is None and not darknet:
        bn_eps = net_utils.read_yolov2_bn_eps(latest)
    if rec is not None:
        trainer = yolov2.YOLOv2DarknetTrainer.from_cfg(rec, args.batch, first, dtype=args.dtype, seed=args.seed,
                                                       solver=args.solver_record, prior_images=args.prior_images,
                                                       tree=args.tree_record, tree_thresh=args.hier_thresh,
                                                       wide_head=getattr(args, "wide_head", False))
    else:
        trainer = TRAINERS[args.topology](args.batch, first, num_class=imdb.num_class, anchors=anchors, dtype=args.dtype,
                                          seed=args.seed, width_div=args.width_div, area_weight=args.area_weight,
                                          prior_images=args.prior_images, solver=args.solver_record, bn_eps=bn_eps,
                                          topology=args.topology, tree=args.tree_record, tree_thresh=args.hier_thresh)
    last_iter_num = 0
    if latest:
        print('Restorining model snapshots from {:s}'.format(latest))
        last_iter_num = net_utils.restore_yolov2_snapshot(trainer, latest)
        skip_batches(imdb, last_iter_num)
    elif args.darknet_weights:
        seen = net_utils.load_darknet_weights(trainer, args.darknet_weights)
        print('Model restored from Darknet weight file {:s} ({:d} images seen)'.format(args.darknet_weights, seen))
    elif args.imagenet_ckpt_dir:
        prior = net_utils.get_ordered_ckpts(args.imagenet_ckpt_dir, 'darknet19', True)
        if prior:
            net_utils.load_darknet19_backbone(trainer, net_utils.read_darknet19_core(prior[-1]))
            print('Backbone restored from {:s}'.format(prior[-1]))
    elif args.darknet_backbone and darknet:
        n = net_utils.load_darknet_prefix(trainer, args.darknet_backbone)
        print('{:d} layers restored from Darknet weight file {:s}'.format(n, args.darknet_backbone))
    elif args.darknet_backbone:
        net_utils.load_darknet19_backbone(trainer, net_utils.read_darknet_backbone(args.darknet_backbone, trainer.bn_eps,
                                                                                   width_div=args.width_div))
        print('Backbone restored from Darknet weight file {:s}'.format(args.darknet_backbone))
    TOTAL_ITER = args.iters + last_iter_num
    T = Timer()
    T.tic()
    losses, sizes = [], []
    stats = torch.empty(6, dtype=torch.float32, device="cuda") if args.region_stats else None
    region_stats = [] if args.region_stats else None
    for i in range(last_iter_num + 1, TOTAL_ITER + 1):
        size = step_size(args, i)
        if args.box_labels:
            image, _grid, truth, ntruth = imdb.get(size)      # three kernels on this stream, no host pixel work
            loss = trainer.step(image, truth=truth, ntruth=ntruth, stats=stats)
        else:
            image, gt_labels = imdb.get(size)                 # two kernels on this stream, no host pixel work
            loss = trainer.step(image, gt_labels)
        losses.append(loss.cpu().numpy().copy())              # coord, object, noobject, class, total
        sizes.append(size)
        if stats is not None:
            region_stats.append(stats.cpu().numpy().copy())    # avg IoU, class, obj, no obj, avg recall, count
        if i % 10 == 0:
            _time = T.toc(average=False)
            rate = ''
            if args.solver_record is not None:
                from ..utils.solver import current_rate
                # of the host's iteration number: after a skipped step the device's counter, the one applied, is behind
                rate = ', rate of iteration {:d}: {:.3e}'.format(i, float(current_rate(args.solver_record, i)))
            print('iter {:d}/{:d}, size {:d}, total loss: {:.3}{:s}, take {:.2}s'.format(i, TOTAL_ITER, size,
                                                                                        float(losses[-1][4]), rate, _time))
            if stats is not None:
                from ..utils.region_loss import REGION_STATS_LINE
                r = region_stats[-1]
                print(REGION_STATS_LINE % (r[0], r[1], r[2], r[3], r[4], int(r[5])))
            T.tic()
        if args.ckpt_dir and (i % args.save_every == 0 or i == TOTAL_ITER):
            print("Model saved in file: %s" % net_utils.save_yolov2_snapshot(trainer, args.ckpt_dir, i))
    torch.cuda.synchronize()
    return {"losses": losses, "last_iter": TOTAL_ITER, "first_iter": last_iter_num + 1, "trainer": trainer,
            "sizes": sizes, "anchors": np.asarray(anchors, np.float32), "imdb": imdb, "topology": args.topology,
            "region_stats": region_stats}


if __name__ == "__main__":
    main()
