"""Counterpart of src/imagenet/imagenet_test_darknet.py: validation accuracy with per-batch timing.
    python -m tensorflow_yolo2_amd.imagenet.imagenet_test_darknet --image-list val.txt --ckpt-dir DIR [--batch 50] [--device-data
        [--views stretch|centre|ten] [--topk 5] [--crop-margin 32]]
darknet19(is_training = 0) -> accuracy per batch (:30-34), the latest snapshot restored (:47-51), the loop and the two
summary lines of :53-68 (the image count must be a multiple of the batch size, :21).  --device-data: the list is decoded
once into a device pool (img_dataset/device_cls.DeviceCls) and every batch is its eval_batch, uint8 into the network.

--views / --topk (with --device-data): Darknet's classifier validation.  Every image gives V views (img_dataset/
eval_views.py: the stretch, the aspect-preserving centre crop of validate_classifier_single, or the ten crops of
validate_classifier_10 with --crop-margin), --batch keeps counting IMAGES and the network is built at batch x V; per batch
DeviceCls.eval_views -> forward -> engine.score_views (softmax per view, mean over the views, top-k, the label's rank) into
one counter tensor on the device.  The image count need not be a multiple of the batch (the short last batch repeats its
final entry, which the counters skip), and the summary is top-1 / top-k over the images, not a mean of batch means."""
import argparse

import numpy as np
import torch

from .. import engine as E, synthetic
from ..utils.timer import Timer
from ..yolo2_nets import net_utils
from . import load_batch, read_image_list


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--image-list", default=None)
    ap.add_argument("--batches", type=int, default=2, help="synthetic batches when no list is given")
    ap.add_argument("--batch", type=int, default=50)           # ilsvrc_cls('val', batch_size=50) (:20)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--ckpt-dir", default=None)
    ap.add_argument("--device-data", action="store_true", help="batches from a device-resident pool (needs --image-list)")
    ap.add_argument("--views", default=None, choices=("stretch", "centre", "ten"),
                    help="with --device-data: the evaluation views of every image (img_dataset/eval_views.py)")
    ap.add_argument("--topk", type=int, default=None, help="with --device-data: also the top-k accuracy (5)")
    ap.add_argument("--crop-margin", type=int, default=32, help="--views ten: the short side is scaled to 224 + margin")
    args = ap.parse_args(argv)
    if args.device_data and not args.image_list:
        ap.error("--device-data needs --image-list")
    scored = args.views is not None or args.topk is not None
    if scored and not args.device_data:
        ap.error("--views and --topk need --device-data")
    size = 224
    items = read_image_list(args.image_list) if args.image_list else None
    V = 1
    if scored:
        from ..img_dataset.eval_views import VIEWS
        views, topk = args.views or "stretch", 5 if args.topk is None else args.topk
        if not 1 <= topk <= 8:
            ap.error("--topk %d outside 1..8" % topk)
        if args.crop_margin < 0:
            ap.error("--crop-margin %d below 0" % args.crop_margin)
        V = VIEWS[views]
        total_batch = (len(items) + args.batch - 1) // args.batch
    else:
        if items is not None:
            assert 0 == (len(items) % args.batch)
        total_batch = len(items) // args.batch if items is not None else args.batches
    net = E.Network(list(E.CORE_SPEC) + list(E.CLS_HEAD_SPEC), args.batch * V, size, size, dtype=args.dtype,
                    core_layers=len(E.CORE_SPEC) + len(E.CLS_HEAD_SPEC), tail=E._lib.Y2_TAIL_AVGPOOL, tail_k=size // 32,
                    training=False)
    net.init_params(0)
    if args.ckpt_dir:
        ckpts = net_utils.get_ordered_ckpts(args.ckpt_dir, 'darknet19', save_epoch=True)
        if ckpts:
            print('Restorining model snapshots from {:s}'.format(ckpts[-1]))
            net_utils.restore_variables(net, ckpts[-1], kind="classifier")
            print('Restored.')
    pool = None
    if args.device_data:
        from ..img_dataset.device_cls import DeviceCls
        pool = DeviceCls(items, args.batch)
    T = Timer()
    accumulated_acc = accumulated_time = 0.0
    if scored:
        hits = torch.zeros(4, dtype=torch.int32, device="cuda")
        ranks = torch.empty(total_batch * args.batch, dtype=torch.int32, device="cuda")
        seen = np.zeros(4, np.int64)
        for i in range(total_batch):
            start = i * args.batch
            images, valid = pool.eval_views(size, start, views, margin=args.crop_margin)
            labels = pool.labels_of(start)
            T.tic()
            logits_value = net.forward(images, False, False).contiguous().float()
            E.score_views(logits_value, labels, views=V, k=topk, n_valid=valid, hits=hits,
                          rank=ranks[start:start + args.batch])
            now = hits.cpu().numpy().astype(np.int64)                   # the host read closes the timed region: 16 bytes
            _time = T.toc(average=False)
            d = now - seen
            seen = now
            print("batch {:d}/{:d}, acc: {:3f}, time: {:2f}sec, top-{:d}: {:3f}"
                  .format(i + 1, total_batch, d[1] / float(d[0]), _time, topk, d[2] / float(d[0])))
            accumulated_time += _time
        images_seen = int(seen[0])
        assert images_seen == len(items), (images_seen, len(items))
        top1, topk_acc = seen[1] / float(images_seen), seen[2] / float(images_seen)
        print("###########validation accuracy:", top1)
        print("###########validation top-{:d} accuracy:".format(topk), topk_acc)
        if seen[3]:
            print("###########labels outside the %d classes: %d" % (logits_value.shape[1], seen[3]))
        print("###########average time per batch:", (accumulated_time / float(total_batch)))
        return {"accuracy": top1, "time_per_batch": accumulated_time / float(total_batch), "network": net, "top1": top1,
                "topk": topk_acc, "images": images_seen, "ranks": ranks[:images_seen].cpu().numpy()}
    for i in range(total_batch):
        if pool:
            (images, _valid), labels = pool.eval_batch(size, i * args.batch), pool.labels_of(i * args.batch)
        elif items is not None:
            images, labels = load_batch(items[i * args.batch:(i + 1) * args.batch], size)
        else:
            images, labels = synthetic.images(args.batch, size, i), synthetic.cls_labels(args.batch, i)
        images, labels = torch.as_tensor(images).cuda(), torch.as_tensor(labels).cuda()
        T.tic()
        logits_value = net.forward(images, False, False)
        accuracy_value = float(E.accuracy(logits_value, labels))      # the host read closes the timed region
        _time = T.toc(average=False)
        print("batch {:d}/{:d}, acc: {:3f}, time: {:2f}sec".format(i + 1, total_batch, accuracy_value, _time))
        accumulated_acc += accuracy_value
        accumulated_time += _time
    print("###########validation accuracy:", (accumulated_acc / float(total_batch)))
    print("###########average time per batch:", (accumulated_time / float(total_batch)))
    return {"accuracy": accumulated_acc / float(total_batch), "time_per_batch": accumulated_time / float(total_batch),
            "network": net}


if __name__ == "__main__":
    main()
