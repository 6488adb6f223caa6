"""VOC mAP of the grid detector over an image set (not in the reference, which has no evaluation code):
    python -m tensorflow_yolo2_amd.pascal.pascal_eval_darknet --devkit data/VOCdevkit --image-set test \
        [--weights FILE | --ckpt-dir DIR] [--size 416] [--batch 32] [--metric 07|10]
The graph and the restore are pascal_detect_darknet.py's; the images come from the device-resident pool
(img_dataset.device_voc.DeviceVOC) in list order.  Per batch, four calls on one stream and nothing on the host:
    DeviceVOC.eval_batch (resize) -> forward_u8 -> y2_detect_grid_batch (decode to the pixels of each original image +
    class-aware NMS) -> y2_voc_match_batch (TP / FP / ignored against the image's ground truth, `difficult` included)
The det / score / count / flags of every batch land in ONE device buffer; after the last batch it is copied to the host
once and utils/detect_batch.map_from_flags makes the per-class precision / recall curves (the only part of the protocol
that needs a sort across images) and the APs.

Both parts of the network normalise with the MOVING statistics by default: with batch statistics a detection depends on
the other images of its batch (and the repeated entries that fill the last one).  --head-batch-stats gives the
reference's detect-time behaviour (pascal_detect_darknet.py: the head is built with its default is_training=True).
With neither --weights nor --ckpt-dir the initial values are evaluated: a plumbing run, as the detect script allows."""
import argparse
import os
import sys

import numpy as np
import torch

from .. import config as cfg, engine
from ..img_dataset import pascal_voc
from ..utils import detect_batch
from ..yolo2_nets import darknet, net_utils


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--devkit", required=True, help="VOCdevkit directory (cfg.PASCAL_PATH)")
    ap.add_argument("--image-set", default="test")
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--weights", default=None, help="snapshot file")
    ap.add_argument("--ckpt-dir", default=None, help="directory of train_iter_*.npz snapshots: the latest is evaluated")
    ap.add_argument("--thresh", type=float, default=0.005, help="confidence above which a box is a detection")
    ap.add_argument("--nms", type=float, default=0.45, help="IoU above which a box of the same class is suppressed")
    ap.add_argument("--max-out", type=int, default=100, help="detections kept per image")
    ap.add_argument("--metric", default="07", choices=("07", "10"), help="07: 11-point AP; 10: area under the envelope")
    ap.add_argument("--head-batch-stats", action="store_true",
                    help="the head normalises with batch statistics, as the reference's detect script does")
    ap.add_argument("--keep-predicts", action="store_true", help="return the head outputs of every image (tests)")
    args = ap.parse_args(argv)
    if args.size < 32 or args.size % 32:
        ap.error("--size %d: the detector head needs a positive multiple of 32 (S = size / 32)" % args.size)
    if args.batch < 1 or args.max_out < 1:
        ap.error("--batch and --max-out must be at least 1")
    return args


def main(argv=None):
    args = parse_args(argv)
    from ..img_dataset.device_voc import DeviceVOC
    B, NUM_CLASS = cfg.B, len(pascal_voc.CLASSES)
    S, n, max_out = args.size // 32, args.batch, args.max_out
    darknet.set_default_dtype(args.dtype)
    imdb = DeviceVOC(args.image_set, batch_size=n, devkit_path=args.devkit, flipped=False)
    input_data = torch.empty((n, args.size, args.size, 3), dtype=torch.uint8, device="cuda")
    core_net = darknet.darknet19_core(input_data, is_training=False)
    final_conv_layer = darknet.darknet19_detection(core_net, 5 * B + NUM_CLASS, is_training=args.head_batch_stats)
    grid_net = final_conv_layer.reshape([-1, S, S, 5 * B + NUM_CLASS])
    network = grid_net.build(training=False)
    restored = 0
    if args.weights and os.path.isfile(args.weights):
        print('Restorining model from weight file {:s}'.format(args.weights))
        restored = len(net_utils.restore_variables(network, args.weights)[0])
    elif args.ckpt_dir:
        restored = net_utils.restore_darknet19_variables(network, args.ckpt_dir, net_name='darknet19', save_epoch=False)
    result = evaluate(network, imdb, args.size, args.thresh, args.nms, args.max_out, args.metric == "07",
                      args.head_batch_stats, args.keep_predicts)
    for c in sorted(result["aps"]):
        print('AP for {:s} = {:.4f}'.format(pascal_voc.CLASSES[c], result["aps"][c]))
    print('Mean AP = {:.4f} ({:d} images, {:d} detections, VOC{:s} metric)'.format(
        result["mAP"], len(imdb.entries), len(result["rows"]["flag"]), "07" if args.metric == "07" else "10+"))
    result.update(restored=restored, network=network, imdb=imdb)
    return result


def evaluate(network, imdb, size, thresh=0.005, nms=0.45, max_out=100, use_07_metric=True, head_batch_stats=False,
             keep_predicts=False):
    """one pass over imdb's image list through `network` (a detector Network of imdb.batch_size images of `size`):
    {"mAP", "aps", "rows", "count", "npos"[, "predicts"]}; everything per image runs on the device, one copy at the end"""
    B, NUM_CLASS = cfg.B, len(pascal_voc.CLASSES)
    S, n = size // 32, imdb.batch_size
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
    predicts = torch.empty((N, S, S, 5 * B + NUM_CLASS), dtype=torch.float32, device="cuda") if keep_predicts else None
    difficult = imdb.difficult
    for k in range(batches):
        lo = k * n
        images, _valid = imdb.eval_batch(size, lo)
        out = grid_net_forward(network, images, head_batch_stats, predicts[lo:lo + n] if predicts is not None else None)
        out = out.view(n, S, S, 5 * B + NUM_CLASS)
        engine.detect_grid_batch(out, imdb.table, imdb.eval_index, NUM_CLASS, B, thresh, nms, max_out,
                                 out=(det[lo:lo + n], score[lo:lo + n], count[lo:lo + n]))
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
    if predicts is not None:
        result["predicts"] = predicts[:entries]
    return result


def grid_net_forward(network, images, head_batch_stats, out=None):
    """one forward pass of the detector on a uint8 BGR batch: the core on its moving statistics, the head too unless
    head_batch_stats"""
    return network.forward(images, False, bool(head_batch_stats), out=out)


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
