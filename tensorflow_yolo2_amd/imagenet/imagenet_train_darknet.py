"""Counterpart of src/imagenet/imagenet_train_darknet.py:
    python -m tensorflow_yolo2_amd.imagenet.imagenet_train_darknet --iters 20 [--image-list train.txt --val-list val.txt]
        [--device-data [--augment [--angle 7 --crop-chance .75 --hue .1 --saturation 1.5 --exposure 1.5 --fill 127]]
         [--pool-short-side 292] [--val-views stretch|centre|ten]] [--size 224]
Graph as the reference (:46-61): darknet19(input, is_training) -> sparse_softmax_cross_entropy_with_logits ->
reduce_mean -> MomentumOptimizer(0.001, 0.9); accuracy = mean(argmax == label).  Loop as the reference (:87-135): restore
the latest `train_epoch_<e>` snapshot (variables and Momentum slots; the reference requires one -- here a fresh tree
starts from the initial values), print loss / accuracy / time every step, a validation batch with is_training = 0 every
25 steps, a snapshot at the end of every --save-every steps.

--device-data (needs --image-list): the decoded list lives in device memory (img_dataset/device_cls.DeviceCls) and every
train batch is one launch -- with --augment the mirror / rotation / scale / crop / colour of img_dataset/augment_cls.py,
else the plain stretch; the uint8 batch goes to ClassifierTrainer.step as it is (Network.forward converts on the device).
The validation batch walks --val-list in list order through a second pool's eval_batch.  --pool-short-side L0 stores
larger images with a short side of L0; --val-views centre | ten scores the validation batch on evaluation views
(img_dataset/eval_views.py, averaged by engine.score_views) in place of the stretch.  Without --device-data nothing changes."""
import argparse
import os
import re

import numpy as np
import torch

from .. import config as cfg, engine as E, synthetic
from ..trainer import ClassifierTrainer
from ..utils.timer import Timer
from ..yolo2_nets import net_utils
from . import load_batch, read_image_list


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)           # ilsvrc_cls('train', batch_size=...) of the reference run
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--ckpt-dir", default=None, help="cfg.get_ckpts_dir('darknet19', imdb.name)")
    ap.add_argument("--ckpt-format", default="npz", choices=("npz", "ckpt"))
    ap.add_argument("--save-every", type=int, default=0, help="steps between snapshots (the reference: every 2 epochs)")
    ap.add_argument("--image-list", default=None, help="training images: lines `path label`")
    ap.add_argument("--val-list", default=None)
    ap.add_argument("--size", type=int, default=224, help="input size, a multiple of 32 (448: the high-resolution fine-tune)")
    ap.add_argument("--device-data", action="store_true", help="batches from a device-resident pool (needs --image-list)")
    ap.add_argument("--augment", action="store_true", help="with --device-data: img_dataset/augment_cls.ClsAugment")
    ap.add_argument("--angle", type=float, default=7.0)
    ap.add_argument("--crop-chance", type=float, default=0.75)
    ap.add_argument("--hue", type=float, default=0.1)
    ap.add_argument("--saturation", type=float, default=1.5)
    ap.add_argument("--exposure", type=float, default=1.5)
    ap.add_argument("--fill", type=int, default=127)
    ap.add_argument("--pool-short-side", type=int, default=None)
    ap.add_argument("--val-views", default="stretch", choices=("stretch", "centre", "ten"),
                    help="with --device-data and --val-list: the views of a validation image (stretch: eval_batch)")
    ap.add_argument("--seed", type=int, default=0, help="with --device-data: the batch order and the augmentation stream")
    args = ap.parse_args(argv)
    if args.device_data and not args.image_list:
        ap.error("--device-data needs --image-list")
    if (args.augment or args.pool_short_side is not None) and not args.device_data:
        ap.error("--augment and --pool-short-side need --device-data")
    if args.val_views != "stretch" and not (args.device_data and args.val_list):
        ap.error("--val-views needs --device-data and --val-list")
    size = args.size
    if size < 32 or size % 32:
        ap.error("--size %d is not a positive multiple of 32" % size)
    tr = ClassifierTrainer(args.batch, size, dtype=args.dtype)
    old_epoch = 0
    if args.ckpt_dir:
        os.makedirs(args.ckpt_dir, exist_ok=True)
        ckpts = net_utils.get_ordered_ckpts(args.ckpt_dir, 'darknet19', save_epoch=True)
        if ckpts:
            print('Restorining model snapshots from {:s}'.format(ckpts[-1]))
            net_utils.restore_variables(tr.net, ckpts[-1], kind="classifier", optimizer=tr.opt)
            print('Restored.')
            old_epoch = int(re.search(r"_(\d+)\.(npz|ckpt)$", ckpts[-1]).group(1))
    train = read_image_list(args.image_list) if args.image_list else None
    val = read_image_list(args.val_list) if args.val_list else None
    pool = vpool = None
    if args.device_data:
        from ..img_dataset.augment_cls import ClsAugment
        from ..img_dataset.device_cls import DeviceCls
        aug = ClsAugment(angle=args.angle, crop_chance=args.crop_chance, hue=args.hue, saturation=args.saturation,
                         exposure=args.exposure, fill=args.fill) if args.augment else None
        pool = DeviceCls(train, args.batch, seed=args.seed, augment=aug, pool_short_side=args.pool_short_side)
        if val:
            vpool = DeviceCls(val, args.batch, seed=args.seed, pool_short_side=args.pool_short_side)
        vstart = 0
        if vpool and args.val_views != "stretch":
            from ..img_dataset.eval_views import VIEWS
            vviews = VIEWS[args.val_views]
            # the trainer's network is built at the train batch: the views of a validation batch need one of their own,
            # on the trainer's variables and batch-norm state
            vnet = E.Network(tr.net.spec, args.batch * vviews, size, size, dtype=args.dtype,
                             core_layers=tr.net.core_layers, tail=E._lib.Y2_TAIL_AVGPOOL, tail_k=size // 32,
                             training=False, buffers=(tr.net.params, None, tr.net.state))
    epoch = old_epoch + 1
    rng = np.random.default_rng(epoch)
    T = Timer()
    log = []
    for i in range(args.iters):
        T.tic()
        if pool:
            images, labels = pool.get(size)
        elif train:
            pick = [train[j] for j in rng.integers(0, len(train), args.batch)]
            images, labels = load_batch(pick, size)
        else:
            images, labels = synthetic.images(args.batch, size, 10 * epoch + i), synthetic.cls_labels(args.batch, 77 + i)
        images, labels = torch.as_tensor(images).cuda(), torch.as_tensor(labels).cuda()
        loss, logits = tr.step(images, labels)
        loss_value, acc_value = float(loss), float(E.accuracy(logits, labels))
        _time = T.toc(average=False)
        print('epoch {:d}, iter {:d}/{:d}, training loss: {:.3}, training acc: {:.3}, take {:.2}s'
              .format(epoch, i + 1, args.iters, loss_value, acc_value, _time))
        log.append((loss_value, acc_value))
        if (i + 1) % 25 == 0 and val:
            T.tic()
            if vpool and args.val_views != "stretch":
                (vi, _valid), vl = vpool.eval_views(size, vstart, args.val_views), vpool.labels_of(vstart)
                vstart = (vstart + args.batch) % len(val)
                vnet.params_changed()                                       # the optimizer has moved the variables
                vlogits = vnet.forward(vi, False, False).contiguous().float()
                _, _, _, vhits, vprob = E.score_views(vlogits, vl, views=vviews, k=5, want_prob=True)
                vh, vp, lab = vhits.cpu().numpy(), vprob.cpu().numpy(), vl.cpu().numpy()
                # the loss of the averaged prediction, -log p[label], the mean over the batch (host-side reporting)
                with np.errstate(divide="ignore"):                          # (p = 0 in float32: an infinite loss)
                    vloss_value = float(-np.log(vp[np.arange(len(lab)), np.clip(lab, 0, vp.shape[1] - 1)]
                                                .astype(np.float64)).mean())
                print('###validation loss: {:.3}, validation acc: {:.3}, take {:.2}s'
                      .format(vloss_value, vh[1] / float(vh[0]), T.toc(average=False)))
            elif vpool:
                (vi, _valid), vl = vpool.eval_batch(size, vstart), vpool.labels_of(vstart)
                vstart = (vstart + args.batch) % len(val)
            else:
                vi, vl = load_batch([val[j] for j in rng.integers(0, len(val), args.batch)], size)
                vi, vl = torch.as_tensor(vi).cuda(), torch.as_tensor(vl).cuda()
            if not (vpool and args.val_views != "stretch"):
                vlogits = tr.net.forward(vi, False, False)                  # is_training: 0
                vloss, _ = E.softmax_cross_entropy(vlogits, vl, need_grad=False)
                print('###validation loss: {:.3}, validation acc: {:.3}, take {:.2}s'
                      .format(float(vloss), float(E.accuracy(vlogits, vl)), T.toc(average=False)))
        if args.ckpt_dir and ((args.save_every and (i + 1) % args.save_every == 0) or i + 1 == args.iters):
            save_path = os.path.join(args.ckpt_dir, cfg.TRAIN_SNAPSHOT_PREFIX + '_epoch_' + str(epoch) + '.' + args.ckpt_format)
            net_utils.save_variables(tr.net, save_path, kind="classifier", optimizer=tr.opt)
            print("Model saved in file: %s" % save_path)
    return {"log": log, "epoch": epoch, "trainer": tr}


if __name__ == "__main__":
    main()
