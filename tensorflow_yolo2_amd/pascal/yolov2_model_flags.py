"""What pascal_eval_yolov2.py and pascal_detect_yolov2.py share: the flags that name the model, their checks, and the
sequence snapshot -> its anchors, class count and batch-norm epsilon -> YOLOv2Detector -> restore.  The flags are added in
two groups so that each script's usage line keeps its order."""
from ..yolo2_nets import net_utils, yolov2


def add_model_flags(ap, batch, batch_help, latest_is, darknet_classes):
    """--size, --batch, --dtype and the three ways to name the weights.  batch / batch_help: the script's own default and
    help of --batch; latest_is: what happens to the latest snapshot of --ckpt-dir ("evaluated", "used"); darknet_classes:
    where a Darknet file's class count comes from"""
    ap.add_argument("--size", type=int, default=None, help="416, or the width of --cfg")
    ap.add_argument("--batch", type=int, default=batch, help=batch_help)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--weights", default=None, help="snapshot file (train_iter_<i>.npz of pascal_train_yolov2.py)")
    ap.add_argument("--ckpt-dir", default=None, help="directory of train_iter_*.npz snapshots: the latest is " + latest_is)
    ap.add_argument("--darknet-weights", default=None,
                    help="a Darknet .weights file of yolov2-voc.cfg (yolov2-voc.weights) or of tiny-yolo-voc.cfg "
                         "(tiny-yolo-voc.weights): builds the graph the file holds, by its float count -- the \"darknet\" or "
                         "the \"tiny\" topology -- with that graph's published anchors and %s; not with --weights or "
                         "--ckpt-dir" % darknet_classes)
    ap.add_argument("--cfg", default=None,
                    help="the Darknet .cfg file that goes with --darknet-weights: it decides the graph, the class count, the "
                         "anchors and the widths, and the file's float count is checked against it instead of guessed "
                         "from; --size defaults to its width.  Not with --weights, --ckpt-dir or --width-div")
    ap.add_argument("--names", default=None,
                    help="a Darknet .names file, one class name per line: the names the detections are written under.  Its "
                         "line count must be the model's class count")
    add_tree_flags(ap)


def add_tree_flags(ap):
    """--tree and --hier-thresh, next to --cfg in every script that builds a YOLOv2 model"""
    ap.add_argument("--tree", default=None,
                    help="a word-tree file (`label parent` per line; utils/word_tree.py): the classes are its nodes, the "
                         "class softmax runs per group of siblings and a detection is the node where the walk down the "
                         "tree stops.  Beats softmax_tree of --cfg; its node count must be the model's class count")
    ap.add_argument("--hier-thresh", type=float, default=None,
                    help="where a detection's walk down the tree stops, in [0, 1): tree_thresh of --cfg, else 0.5")


def resolve_tree(ap, args):
    """behind the cfg: args.tree_record = the utils.word_tree.WordTree of --tree, else of the cfg's softmax_tree, else
    None; args.hier_thresh = the flag, else the cfg's tree_thresh, else 0.5"""
    from ..utils import word_tree
    rec = args.cfg_record
    args.tree_record = None
    try:
        if args.tree:
            args.tree_record = word_tree.load(args.tree)
        elif rec is not None:
            args.tree_record = yolov2.load_cfg_tree(rec)
    except (OSError, ValueError) as e:
        ap.error("%s: %s" % ("--tree" if args.tree else "--cfg", e))
    if args.hier_thresh is None:
        args.hier_thresh = rec.tree_thresh if rec is not None else 0.5
    if not 0.0 <= args.hier_thresh < 1.0:
        ap.error("--hier-thresh %g: a number in [0, 1)" % args.hier_thresh)
    if rec is not None and args.tree_record is not None and args.tree_record.n != rec.classes:
        ap.error("--tree %s holds %d nodes, --cfg %s has classes=%d" % (args.tree, args.tree_record.n, args.cfg, rec.classes))


def check_tree(error, args, num_class):
    """the tree's nodes are the model's classes"""
    if args.tree_record is not None and args.tree_record.n != num_class:
        error("the word tree %s holds %d nodes, the model has %d classes" % (args.tree_record.path, args.tree_record.n,
                                                                             num_class))


def resolve_cfg(ap, args, wide_head=False):
    """right behind parse_args: --cfg read into args.cfg_record (None without the flag) and the flags nobody gave filled
    from it, then from today's defaults; --names read into args.class_names (None without the flag).  wide_head: the
    keyword of utils/darknet_cfg.py, which the scripts that only run a model pass as True -- YOLO9000's cfg then loads
    (`map=` kept unread, its 28,269-filter last layer as engine.WideHead); kept in args.wide_head for build_detector"""
    args.cfg_record = args.class_names = None
    args.wide_head = bool(wide_head)
    if args.cfg:
        from ..utils import darknet_cfg
        if args.weights or args.ckpt_dir:
            ap.error("--cfg describes a Darknet graph, whose snapshot is the .weights file: not with --weights or --ckpt-dir")
        if args.width_div != 1:
            ap.error("--cfg holds the widths: not with --width-div")
        try:
            args.cfg_record = darknet_cfg.load(args.cfg, wide_head)
            darknet_cfg.compile_graph(args.cfg_record, 1024 if args.dtype == "f32" else darknet_cfg.MAX_OUT_WIDTH,
                                      wide_head)
        except (OSError, ValueError) as e:
            ap.error("--cfg: %s" % e)
        if args.size is None:
            args.size = args.cfg_record.size
    if args.size is None:
        args.size = 416
    resolve_tree(ap, args)
    if args.names:
        from ..utils import darknet_cfg
        try:
            args.class_names = darknet_cfg.read_names(args.names)
        except OSError as e:
            ap.error("--names: %s" % e)


def class_names(ap_error, args, num_class, default):
    """the names the detections are written under: --names (its count must be num_class), else `default`"""
    check_tree(ap_error, args, num_class)
    if args.class_names is None:
        return default
    if len(args.class_names) != num_class:
        ap_error("--names %s holds %d names, the model has %d classes" % (args.names, len(args.class_names), num_class))
    return args.class_names


def add_test_flags(ap):
    ap.add_argument("--width-div", type=int, default=1, help="divide every inner width (tests)")
    ap.add_argument("--keep-grids", action="store_true", help="return the raw head outputs of every image (tests)")


def check_size(ap, args):
    if args.size < 32 or args.size % 32:
        ap.error("--size %d: the detector head needs a positive multiple of 32 (S = size / 32)" % args.size)
    num = args.cfg_record.num if getattr(args, "cfg_record", None) is not None else len(yolov2.ANCHORS_VOC)
    if (args.size // 32) ** 2 * num > 2048:
        ap.error("--size %d: more than 2048 candidates per image" % args.size)


def check_weights(ap, args):
    if args.darknet_weights and (args.weights or args.ckpt_dir):
        ap.error("--darknet-weights goes with neither --weights nor --ckpt-dir")


def find_snapshot(args, num_class):
    """-> (snapshot path or None, anchors, class count, bn_eps) of the model to build: the snapshot's own where --weights
    or --ckpt-dir names one, else the published VOC anchors, `num_class` and the default epsilon (--darknet-weights:
    build_detector takes the published anchors of the graph the file holds)"""
    if args.cfg_record is not None:           # the cfg decides: nothing is guessed from the file's float count
        return None, args.cfg_record.anchors, args.cfg_record.classes, None
    snapshot = args.weights
    if not snapshot and args.ckpt_dir:
        sfiles = net_utils.get_ordered_yolov2_ckpts(args.ckpt_dir)
        snapshot = sfiles[-1] if sfiles else None
    if not snapshot:
        return None, yolov2.ANCHORS_VOC, num_class, None
    anchors, num_class, _it = net_utils.read_yolov2_meta(snapshot)
    return snapshot, anchors, num_class, net_utils.read_yolov2_bn_eps(snapshot)


def build_detector(args, snapshot, anchors, num_class, bn_eps):
    """the detector of find_snapshot's answer, filled from --darknet-weights or from the snapshot -> (detector, the
    snapshot's iteration or 0)"""
    check_tree(args.error, args, num_class)
    if args.cfg_record is not None:
        try:
            detector = yolov2.YOLOv2Detector.from_cfg(args.cfg_record, args.batch, args.size, dtype=args.dtype,
                                                      tree=args.tree_record, tree_thresh=args.hier_thresh,
                                                      wide_head=getattr(args, "wide_head", False))
        except ValueError as e:                   # a wide head under --dtype f32 / f16x2 / f16x2f
            args.error("--cfg: %s" % e)
        if args.darknet_weights:
            print('Restorining model from Darknet weight file {:s} (cfg {:s}, topology {:s})'.format(
                args.darknet_weights, args.cfg, detector.topology))
            print('{:d} images seen'.format(net_utils.load_darknet_weights(detector, args.darknet_weights)))
        return detector, 0
    topology = "paper"
    if args.darknet_weights:
        topology = net_utils.darknet_file_topology(args.darknet_weights, num_class, len(anchors), args.width_div)
        anchors = yolov2._TOPOLOGY[topology].anchors
    detector = yolov2.YOLOv2Detector(args.batch, args.size, num_class=num_class, anchors=anchors, dtype=args.dtype,
                                     width_div=args.width_div, bn_eps=bn_eps, topology=topology, tree=args.tree_record,
                                     tree_thresh=args.hier_thresh)
    restored = 0
    if args.darknet_weights:
        print('Restorining model from Darknet weight file {:s} (topology {:s})'.format(args.darknet_weights, topology))
        seen = net_utils.load_darknet_weights(detector, args.darknet_weights)
        print('{:d} images seen'.format(seen))
    if snapshot:
        print('Restorining model from weight file {:s}'.format(snapshot))
        restored = net_utils.restore_yolov2_variables(detector, snapshot)
    return detector, restored
