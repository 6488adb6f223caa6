"""Drop-in counterparts of the hot-path half of src/yolo2_nets/net_utils.py:
    get_iou(boxes1, boxes2, scope='iou')                                           (:222-260)
    get_loss(net, labels, num_class, batch_size, image_size, S, B, OFFSET,
             scope='loss_layer') -> (loss, ious, object_mask)                      (:263-372)
    show_yolo_detection(image_path, predict_output, imdb, object_thresh=0.5)       (:375-439)
All arithmetic runs in the fused HIP kernels of csrc/loss.hip through the C ABI."""
import numpy as np
import torch

from .. import config as cfg
from .. import engine
from .darknet import NetTensor


def get_iou(boxes1, boxes2, scope='iou'):
    """boxes: [..., 4] = (x_center, y_center, w, h) device tensors -> IoU [...]."""
    return engine.get_iou(boxes1, boxes2)


class Loss(torch.Tensor):
    """The scalar `loss` tensor of the reference, remembering what tf.gradients would need."""
    pass


def get_loss(net, labels, num_class, batch_size, image_size, S, B, OFFSET, scope='loss_layer'):
    """Returns (loss, ious, object_mask) like the reference.  `loss` is a 0-d tensor carrying
    `.parts` (class, object, noobject, coord losses), `.dnet` (d loss / d net) and `.source`
    (the NetTensor it came from) so that an optimizer's minimize(loss) can run the backward."""
    expect = cfg.yolo_grid_offset(S, B)
    if np.asarray(OFFSET).shape != expect.shape or not (np.asarray(OFFSET) == expect).all():
        raise ValueError("OFFSET must be the [S,S,B] column-index grid of config.py:40-42")
    source = net if isinstance(net, NetTensor) else None
    # batch statistics, no moving-statistics update yet: the reference's UPDATE_OPS hang off train_op
    # (pascal_train_darknet.py:49-51), so a loss that is only evaluated leaves them alone
    value = net.run(training=True, update_moving=False) if source is not None else net
    if not torch.is_tensor(labels):
        labels = torch.as_tensor(np.asarray(labels, np.float32))
    labels = labels.to(value.device, torch.float32)
    loss5, ious, mask, dnet = engine.yolo_loss(value, labels, num_class, batch_size, image_size, S, B,
                                               need_grad=True, lambda_coord=float(cfg.LAMBDA_COORD),
                                               lambda_noobj=float(cfg.LAMBDA_NOOBJ))
    loss = loss5[4].as_subclass(Loss)
    loss.parts = dict(class_loss=loss5[0], object_loss=loss5[1], noobject_loss=loss5[2], coord_loss=loss5[3])
    loss.dnet = dnet
    loss.source = source
    return loss, ious, mask


class _Optimizer:
    """tf.train.*Optimizer().minimize(loss): returns a train op; calling it applies one update (the BN
    moving-statistics update of the forward that produced `loss`, backward through that stack, then the
    optimizer).  Slots live with the variable store, so every graph sharing the scopes trains ONE state."""
    _engine_cls = None

    def __init__(self, *args):
        self.args = args
        self._opt = {}
        self._reducers = {}

    def _reducer(self, net):
        """data parallelism (trainer.GradReducer): the sliced, overlapped SUM all-reduce of `net`'s gradient buffer"""
        from ..trainer import GradReducer
        r = self._reducers.get(id(net))
        if r is None:
            r = self._reducers[id(net)] = GradReducer(net)
        return r

    def slots(self, net):
        """the engine optimizer (slot tensors) that train ops of this object apply to `net`'s variables"""
        return self._slots(net)

    def _slots(self, net):
        store = getattr(net, "store", None)
        key = id(store) if store is not None else id(net)
        opt = self._opt.get(key)
        if opt is None:
            opt = self._opt[key] = self._engine_cls(net, *self.args)
            if store is not None:
                store.optimizers[type(self).__name__] = opt
        if opt.net is not net:                 # same flat buffers, another context (batch / size)
            assert opt.net.n_params == net.n_params, "one optimizer per variable chain"
            opt.net = net
            if opt.scaler is not None:
                opt.scaler.attach(net)
        return opt

    def minimize(self, loss):
        def train_op(loss=loss):
            src = loss.source
            if src is None or src.network is None or not src.network.training:
                raise RuntimeError("loss was not produced by a training-mode NetTensor")
            net = src.network
            net.update_moving_stats()          # tf.control_dependencies(update_ops)
            from ..trainer import _dist
            if _dist() is None:
                net.backward(loss.dnet.contiguous())
                self._slots(net).step()
            else:
                # one process per GPU under torch.distributed (pascal_train_darknet.py under torchrun): the replicas'
                # gradients are summed slice by slice behind the backward pass and the update divides by the world
                # size -- slim's clone semantics (src/slim_dir/deployment/model_deploy.py:222-225,436-446)
                world = self._reducer(net).backward_and_reduce(loss.dnet.contiguous())
                self._slots(net).step(grad_mult=1.0 / world)
            store = getattr(net, "store", None)
            if store is not None:
                store.version += 1
                # the fused update re-packed THIS context's filter copies already: only the other graphs on the
                # store need the re-pack the version bump asks for (it re-reads every parameter: 193 MB per step)
                opt = self._slots(net)
                if getattr(opt, "fused_pack", False) and net.training:
                    net._seen_version = store.version
        return train_op


class AdamOptimizer(_Optimizer):
    """tf.train.AdamOptimizer().minimize(loss) (pascal_train_darknet.py:51)"""
    _engine_cls = engine.AdamOptimizer

    def __init__(self, learning_rate=0.001, beta1=0.9, beta2=0.999, epsilon=1e-08):
        _Optimizer.__init__(self, learning_rate, beta1, beta2, epsilon)


class MomentumOptimizer(_Optimizer):
    """tf.train.MomentumOptimizer(0.001, 0.9).minimize(loss) (imagenet_train_darknet.py:58)"""
    _engine_cls = engine.MomentumOptimizer

    def __init__(self, learning_rate, momentum):
        _Optimizer.__init__(self, learning_rate, momentum)


def decode_yolo_detection(predict_output, im_w, im_h, num_class, S=cfg.S, B=cfg.B, object_thresh=0.5):
    """The arithmetic of show_yolo_detection (:393-421) on the GPU; returns the reference's
    (upper_left_x, upper_left_y, w, h, class_index, confidence, c, r, i) tuples in loop order."""
    if not torch.is_tensor(predict_output):
        predict_output = torch.as_tensor(np.asarray(predict_output, np.float32)).cuda()
    return engine.decode_detections(predict_output, S, B, num_class, im_w, im_h, object_thresh)


def show_yolo_detection(image_path, predict_output, imdb, object_thresh=0.5, show=True):
    """Compute bounding boxes from the yolo detection network prediction, print them like the
    reference and (when matplotlib + PIL are importable and show=True) draw them."""
    from PIL import Image
    im = np.array(Image.open(image_path), dtype=np.uint8)
    im_h, im_w = im.shape[0], im.shape[1]
    dets = decode_yolo_detection(predict_output, im_w, im_h, imdb.num_class, cfg.S, cfg.B, object_thresh)
    for (ulx, uly, w, h, cls, conf, _c, _r, _i) in dets:
        print("predicted bounding boxes: ({:d}, {:d}), width:{:d}, height:{:d}".format(ulx, uly, w, h))
    if show:
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
            import matplotlib.patches as patches
            fig, ax = plt.subplots(1)
            ax.imshow(im)
            for (ulx, uly, w, h, cls, conf, _c, _r, _i) in dets:
                ax.add_patch(patches.Rectangle((ulx, uly), w, h, linewidth=1, edgecolor='r', facecolor='none'))
                ax.text(ulx, uly, imdb.classes[int(cls)] + ":" + str(np.float32(conf)), color='r')
            fig.savefig("yolo_detection.png")
            plt.close(fig)
        except ImportError:
            pass
    return dets


# ---------------------------------------------------------------------------
# snapshots keyed by the reference's TF variable names (the counterpart of
# get_ordered_ckpts / restore_darknet19_variables, src/yolo2_nets/net_utils.py:14-110).
# Two file formats, same names and contents: `.npz` (numpy) and `.ckpt` = TensorFlow's V2 checkpoint
# (`<prefix>.index` + `<prefix>.data-00000-of-00001`, utils/tf_bundle.py: read and written without TensorFlow), so
# that the checkpoints the reference's tf.train.Saver writes -- and the author's published ones (README.md:22-24)
# -- restore into these buffers, and snapshots written here load in the reference.
# ---------------------------------------------------------------------------
import glob
import os
import re

from . import darknet as _darknet
from ..utils import tf_bundle as _bundle


class _BundleSnap:
    """np.load-like view of a TF V2 checkpoint"""

    def __init__(self, prefix):
        self.r = _bundle.BundleReader(prefix)
        self.files = self.r.names()

    def __getitem__(self, name):
        return self.r.get_tensor(name)


def _ckpt_prefix(path):
    """the checkpoint prefix if `path` names a TF V2 checkpoint (prefix, .index or .meta file), else None"""
    for suffix in ("", ".index", ".meta"):
        if suffix and not path.endswith(suffix):
            continue
        prefix = path[:len(path) - len(suffix)] if suffix else path
        if _bundle.is_bundle(prefix):
            return prefix
    return None


class _DictSnap:
    """np.load-like view of a dict of arrays (a V1 checkpoint read whole)"""

    def __init__(self, d):
        self.d = d
        self.files = sorted(d)

    def __getitem__(self, name):
        return self.d[name]


def _open_snapshot(path):
    prefix = _ckpt_prefix(path)
    if prefix:
        return _BundleSnap(prefix)
    if _bundle.is_v1_checkpoint(path):          # single-file tf.train.Saver V1 checkpoint (slim's resnet_v1_50.ckpt)
        return _DictSnap(_bundle.read_checkpoint_v1(path))
    return np.load(path)


def _kind_of(network):
    n = network.num_layers
    return {18: "core", 19: "classifier", 22: "detector"}.get(n, "detector")


def _names(network, kind):
    kind = kind or _kind_of(network)
    return _darknet.variable_names("classifier" if kind in ("core", "classifier") else kind,
                                   network.spec[-1][2])[:network.num_layers]


def _slot_views(network, flat):
    """per-layer dict of numpy copies of a flat optimizer slot laid out like the parameters"""
    host = flat.detach().cpu().numpy()
    out = []
    for l in range(network.num_layers):
        o = network._offsets[l]
        shp = network._shapes(l)
        d = {}
        for i, k in enumerate(engine.PARAM_KEYS):
            n = int(np.prod(shp[k]))
            d[k] = host[o[i]:o[i] + n].reshape(shp[k]).copy()
        out.append(d)
    return out


def save_variables(network, path, kind=None, optimizer=None):
    """write what tf.train.Saver() writes for the reference graph, under the TF variable names: every
    parameter and BN moving statistic and -- with `optimizer` (an engine Adam/Momentum optimizer) -- its slots
    (`<var>/Adam`, `<var>/Adam_1`, `beta1_power`, `beta2_power`; `<var>/Momentum`), so that a resumed run
    does not restart Adam at t = 0 with empty moments (pascal_train_darknet.py:83,88,111-114)."""
    names = _names(network, kind)
    blob = {}
    for layer, nm in zip(network.export_params(), names):
        for k, tfname in nm.items():
            blob[tfname] = layer[k]
    if optimizer is not None:
        st = optimizer.export_state()
        if "m" in st:
            flat_m = torch.as_tensor(st["m"])
            flat_v = torch.as_tensor(st["v"])
            for lm, lv, nm in zip(_slot_views(network, flat_m), _slot_views(network, flat_v), names):
                for k in engine.PARAM_KEYS:
                    blob[nm[k] + "/Adam"] = lm[k]
                    blob[nm[k] + "/Adam_1"] = lv[k]
            # TF1's Adam creates beta^1 and multiplies once per apply: after t steps the variables hold beta^(t+1)
            blob["beta1_power"] = np.float32(np.float64(optimizer.b1) ** (st["t"] + 1))
            blob["beta2_power"] = np.float32(np.float64(optimizer.b2) ** (st["t"] + 1))
            blob["adam_step"] = np.int64(st["t"])       # authoritative here (not a TF variable)
        else:
            for la, nm in zip(_slot_views(network, torch.as_tensor(st["accum"])), names):
                for k in engine.PARAM_KEYS:
                    blob[nm[k] + "/Momentum"] = la[k]
    if path.endswith(".ckpt"):
        _bundle.write_bundle(path, {k: np.asarray(v) for k, v in blob.items()})
    else:
        np.savez(path, **blob)
    return sorted(blob)


_F32_MIN_NORMAL = 1.1754943508222875e-38


def adam_step_from_powers(beta1_power=None, beta2_power=None, b1=0.9, b2=0.999):
    """Step count t of a TF-written Adam checkpoint, which only holds `beta1_power` = b1^(t+1) and `beta2_power` =
    b2^(t+1) as float32 variables.  b1^(t+1) leaves the normal float32 range after ~830 steps and is 0.0 after ~1000
    (the reference saves at 40000), so the slowly decaying b2 power is used while it is a normal float32 (t < ~87000);
    beyond both, the bias corrections are 1 to float precision and any large t gives the same update."""
    for power, b in ((beta2_power, b2), (beta1_power, b1)):
        if power is None:
            continue
        v = float(np.asarray(power).reshape(-1)[0])
        if np.isfinite(v) and _F32_MIN_NORMAL <= v < 1.0 and 0.0 < b < 1.0:
            return max(0, int(round(np.log(v) / np.log(b))) - 1)
        if np.isfinite(v) and v >= 1.0:
            return 0
    have = [p for p in (beta1_power, beta2_power) if p is not None]
    return 10 ** 6 if have else 0


def restore_variables(network, path, kind=None, optimizer=None):
    """`path`: an .npz snapshot or a TF V2 checkpoint (prefix `x.ckpt`, or its `.index` / `.meta` file name).
    load the variables whose names are present in the snapshot, leave the others as they are
    (the reference restores the ImageNet-trained backbone into the detector this way, :83-103).
    A variable present with another shape raises (tf.train.Saver does too).  With `optimizer`, its slots
    are restored when the snapshot holds them.  Returns (restored names, names left untouched)."""
    names = _names(network, kind)
    snap = _open_snapshot(path)
    layers = network.export_params()
    restored, kept = [], []
    for layer, nm in zip(layers, names):
        for k, tfname in nm.items():
            if tfname in snap.files:
                if tuple(snap[tfname].shape) != tuple(layer[k].shape):
                    raise ValueError("snapshot %s: %s has shape %s, the graph expects %s" %
                                     (path, tfname, tuple(snap[tfname].shape), tuple(layer[k].shape)))
                layer[k] = snap[tfname]
                restored.append(tfname)
            else:
                kept.append(tfname)
    network.load_params(layers)
    if optimizer is not None:
        st = optimizer.export_state()
        if "m" in st and all((nm["W"] + "/Adam") in snap.files for nm in names):
            for slot, suffix in (("m", "/Adam"), ("v", "/Adam_1")):
                flat = st[slot]
                for l, nm in enumerate(names):
                    o = network._offsets[l]
                    for i, k in enumerate(engine.PARAM_KEYS):
                        a = snap[nm[k] + suffix]
                        flat[o[i]:o[i] + a.size] = a.reshape(-1)
            if "adam_step" in snap.files:
                st["t"] = int(snap["adam_step"])
            else:   # a checkpoint written by TF only has the beta powers: beta^(t+1) after t steps
                st["t"] = adam_step_from_powers(snap["beta1_power"] if "beta1_power" in snap.files else None,
                                                snap["beta2_power"] if "beta2_power" in snap.files else None,
                                                optimizer.b1, optimizer.b2)
            optimizer.load_state(st)
        elif "accum" in st and all((nm["W"] + "/Momentum") in snap.files for nm in names):
            flat = st["accum"]
            for l, nm in enumerate(names):
                o = network._offsets[l]
                for i, k in enumerate(engine.PARAM_KEYS):
                    a = snap[nm[k] + "/Momentum"]
                    flat[o[i]:o[i] + a.size] = a.reshape(-1)
            optimizer.load_state(st)
    return restored, kept


def get_ordered_ckpts(ckpt_dir, net_name='darknet19', save_epoch=True):
    """snapshot files of `net_name` in `ckpt_dir`, oldest first (reference :14-38 orders by mtime;
    the number in the name breaks ties of files written within one clock tick)"""
    tag = "epoch" if save_epoch else "iter"
    # reference :27-28: cfg.TRAIN_SNAPSHOT_PREFIX + '_' + save_interval + '_*.ckpt.meta' inside
    # cfg.get_ckpts_dir(net_name, imdb.name); here the caller passes that directory
    stem = os.path.join(ckpt_dir, "%s_%s_*" % (cfg.TRAIN_SNAPSHOT_PREFIX, tag))
    files = glob.glob(stem + ".npz") + [f[:-len(".index")] for f in glob.glob(stem + ".ckpt.index")]

    def key(f):
        m = re.search(r"_(\d+)\.(npz|ckpt)$", f)
        stamp = os.path.getmtime(f if f.endswith(".npz") else f + ".index")
        return (stamp, int(m.group(1)) if m else 0)
    return sorted(files, key=key)


def restore_darknet19_variables(network, ckpt_dir, net_name='darknet19', save_epoch=True, imagenet_ckpt_dir=None,
                                optimizer=None):
    """Reference :64-110: restore the latest snapshot and return its epoch / iteration number; with no
    snapshot, restore what an ImageNet-classifier snapshot holds (the backbone) and return 0."""
    sfiles = get_ordered_ckpts(ckpt_dir, net_name, save_epoch)
    if not sfiles:
        if imagenet_ckpt_dir:
            prior = get_ordered_ckpts(imagenet_ckpt_dir, net_name, True)
            if prior:
                restore_variables(network, prior[-1])
        return 0
    restore_variables(network, sfiles[-1], optimizer=optimizer)
    m = re.search(r"_(\d+)\.(npz|ckpt)$", sfiles[-1])
    return int(m.group(1)) if m else 0


# ---------------------------------------------------------------------------
# ResNet-50 swap (yolo2_nets/tf_resnet.py: ResNet50Yolo): the counterpart of restore_resnet_tf_variables
# (src/yolo2_nets/net_utils.py:137-219).  TF names: the backbone lives under the scope `resnet_v1_50/`, the head
# (`yolo_fc1`, `yolo_fc2`) at the root; Adam slots `<var>/Adam`, `<var>/Adam_1`, `beta1_power`, `beta2_power`.
# ---------------------------------------------------------------------------
RESNET_SCOPE = "resnet_v1_50/"
RESNET_HEAD_SCOPES = ("yolo_fc1", "yolo_fc2", "loss_layer")        # reference :177-186: excluded from the backbone restore


def resnet_tf_name(name):
    return name if name.split("/")[0] in RESNET_HEAD_SCOPES else RESNET_SCOPE + name


def save_resnet_variables(model, path, with_optimizer=True):
    """what tf.train.Saver() writes for the ResNet graph: every variable (moving statistics included) and the Adam
    slots, `.npz` or a TF V2 checkpoint (`.ckpt`)"""
    blob = {}
    if getattr(model, "graph", False):
        model._follow_ctrl()
    m_host = model.m.detach().cpu().numpy() if with_optimizer else None
    v_host = model.v.detach().cpu().numpy() if with_optimizer else None
    for (name, shape, trainable) in model.vars:
        tfname = resnet_tf_name(name)
        blob[tfname] = model.p[name].detach().cpu().numpy().copy()
        if trainable:
            t_off, n = model.offset[name]                   # the flat layout may hold slots that are not variables
            if with_optimizer:
                blob[tfname + "/Adam"] = m_host[t_off:t_off + n].reshape(shape).copy()
                blob[tfname + "/Adam_1"] = v_host[t_off:t_off + n].reshape(shape).copy()
    if with_optimizer:
        blob["beta1_power"] = np.float32(np.float64(0.9) ** (model.t + 1))       # TF1: beta^(t+1) after t applies
        blob["beta2_power"] = np.float32(np.float64(0.999) ** (model.t + 1))
        blob["adam_step"] = np.int64(model.t)
    if path.endswith(".ckpt"):
        _bundle.write_bundle(path, {k: np.asarray(v) for k, v in blob.items()})
    else:
        np.savez(path, **blob)
    return sorted(blob)


def restore_resnet_variables(model, path, exclude=(), with_optimizer=True):
    """load the variables of `path` (.npz, TF V2 prefix, or a single-file V1 checkpoint such as slim's
    resnet_v1_50.ckpt) that the graph has and whose scope is not in `exclude`; shapes must match.  Adam slots and the
    step count are restored when the file holds all of them.  Returns (restored names, names left as they were)."""
    snap = _open_snapshot(path)
    have = set(snap.files)
    restored, kept = [], []
    for (name, shape, _t) in model.vars:
        tfname = resnet_tf_name(name)
        if name.split("/")[0] in exclude or tfname not in have:
            kept.append(tfname)
            continue
        a = np.asarray(snap[tfname], np.float32)
        if tuple(a.shape) != tuple(shape):
            raise ValueError("snapshot %s: %s has shape %s, the graph expects %s" % (path, tfname, tuple(a.shape), tuple(shape)))
        model.p[name].copy_(torch.as_tensor(a).to(model.p[name].device))
        restored.append(tfname)
    trainable = [(n, sh) for (n, sh, t) in model.vars if t]
    if with_optimizer and all(resnet_tf_name(n) + "/Adam" in have and resnet_tf_name(n) + "/Adam_1" in have
                              for n, _ in trainable):
        m_host = np.zeros(model.m.numel(), np.float32)
        v_host = np.zeros(model.v.numel(), np.float32)
        for n, sh in trainable:
            off, k = model.offset[n]
            m_host[off:off + k] = np.asarray(snap[resnet_tf_name(n) + "/Adam"], np.float32).reshape(-1)
            v_host[off:off + k] = np.asarray(snap[resnet_tf_name(n) + "/Adam_1"], np.float32).reshape(-1)
        model.m.copy_(torch.as_tensor(m_host).to(model.m.device))
        model.v.copy_(torch.as_tensor(v_host).to(model.v.device))
        if "adam_step" in have:
            t = int(snap["adam_step"])
        else:
            t = adam_step_from_powers(snap["beta1_power"] if "beta1_power" in have else None,
                                      snap["beta2_power"] if "beta2_power" in have else None)
        model.t = t
        model.ctrl[1] = t                               # the guarded update keeps its step count on the device
    if hasattr(model, "params_changed"):
        model.params_changed()                          # fused stacks re-pack their filters from the restored values
    return restored, kept


def restore_resnet_tf_variables(model, ckpt_dir, net_name='resnet50', retrain=False, detection=True, save_epoch=True,
                                new_optimizer=None, weights_path=None):
    """Reference :137-219.  No snapshot in `ckpt_dir`: the head and the optimizer keep their initial values and the
    convolutional layers are restored from the downloaded `resnet_v1_50.ckpt` under `weights_path` (cfg.WEIGHTS_PATH;
    skipped when the file is absent) -> 0.  Otherwise the latest snapshot is restored (without its optimizer slots
    when `new_optimizer` names a new optimizer) -> its iteration / epoch number.
    Difference from the reference: its `retrain` argument is accepted and IGNORED there (:137-219 never reads it); here
    `retrain=True` skips the snapshots and starts again from the downloaded backbone weights, as the name says.  The
    default (False) is the reference's behaviour."""
    sfiles = get_ordered_ckpts(ckpt_dir, net_name, save_epoch) if ckpt_dir else []
    if not sfiles or retrain:
        if weights_path:
            f = weights_path if os.path.isfile(weights_path) or _ckpt_prefix(weights_path) else \
                os.path.join(weights_path, "resnet_v1_50.ckpt")
            if os.path.isfile(f) or _ckpt_prefix(f):
                print('Initializing new variables to train from downloaded resnet50 weights')
                restore_resnet_variables(model, f, exclude=RESNET_HEAD_SCOPES if detection else (), with_optimizer=False)
        return 0
    print('Restorining model snapshots from {:s}'.format(sfiles[-1]))
    restore_resnet_variables(model, sfiles[-1], with_optimizer=new_optimizer is None)
    print('Restored.')
    m = re.search(r"_(\d+)\.(npz|ckpt)$", sfiles[-1])
    return int(m.group(1)) if m else 0


# ---------------------------------------------------------------------------
# YOLOv2 (yolo2_nets/yolov2.py: YOLOv2Detector, YOLOv2Trainer; not in the reference): one `.npz` for the three stacks and
# the optimizer of the composed graph.  The names are utils/yolov2_snapshot.py's.
# ---------------------------------------------------------------------------
from ..utils import yolov2_snapshot as _v2snap


def _layer_slots(network, layers):
    """flat float32 array laid out like `network`'s parameters from per-layer dicts of PARAM_KEYS"""
    flat = np.zeros(network.n_params, np.float32)
    for l, d in enumerate(layers):
        o = network._offsets[l]
        for i, k in enumerate(engine.PARAM_KEYS):
            a = np.asarray(d[k], np.float32).reshape(-1)
            flat[o[i]:o[i] + a.size] = a
    return flat


def save_yolov2_variables(model, path, iteration=None):
    """model: a YOLOv2Detector or a YOLOv2Trainer -> one .npz: the parameters and batch-norm state of the three stacks,
    the anchors, the class count and the iteration (default: model.iteration); for a trainer also the three Adam states
    (or, on Darknet's solver, the three Momentum slots and the solver record) and the one loss scaler and step counter
    they share, so that a resumed run continues the uninterrupted one.  A batch-norm epsilon other than the default adds
    the key yolov2/bn_eps.  The "darknet" topology has no .npz form: its snapshot is the .weights file"""
    _refuse_darknet_topology(model, "save_yolov2_variables", "save_darknet_weights")
    nets = model.networks()
    stacks = {s: net.export_params() for s, net in zip(_v2snap.STACKS, nets)}
    adam = scaler = sgd = None
    solver = getattr(model, "solver", None)
    if hasattr(model, "opts"):
        adam, sgd = ({}, None) if solver is None else (None, {})
        for s, net, opt in zip(_v2snap.STACKS, nets, model.opts):
            st = opt.export_state()
            if solver is None:
                adam[s] = {"m": _slot_views(net, torch.as_tensor(st["m"])),
                           "v": _slot_views(net, torch.as_tensor(st["v"])), "t": st["t"]}
            else:
                sgd[s] = {"accum": _slot_views(net, torch.as_tensor(st["accum"])), "t": st["t"]}
        sc = model.opts[0].scaler
        if sc is not None:
            scaler = {"ctrl": sc.ctrl.cpu().numpy(), "scale": sc.scale, "clean": sc._clean}
    blob = _v2snap.to_blob(stacks, model.anchors, model.num_class,
                           model.iteration if iteration is None else iteration, adam, scaler, sgd,
                           solver if sgd is not None else None, bn_eps=getattr(model, "bn_eps", None))
    np.savez(path, **blob)
    return sorted(blob)


def restore_yolov2_variables(model, path):
    """the inverse of save_yolov2_variables -> the snapshot's iteration (also left in model.iteration).  A
    YOLOv2Detector takes the parameters and batch-norm state only; a YOLOv2Trainer also the optimizer when the file
    holds it.  Other anchors, another class count or a tensor of another shape raise, naming both values; so does a
    trainer on one optimizer given the slots of the other, or another solver record than its own, or a model whose
    batch-norm epsilon is not the snapshot's (yolov2/bn_eps; the default where the file has no such key)."""
    _refuse_darknet_topology(model, "restore_yolov2_variables", "load_darknet_weights")
    with np.load(path) as snap:
        stacks, anchors, num_class, iteration, adam, scaler = _v2snap.from_blob(snap)
        sgd, snap_solver = _v2snap.sgd_from_blob(snap)
        snap_eps = _v2snap.bn_eps_from_blob(snap)
    model_eps = getattr(model, "bn_eps", None)
    model_eps = _v2snap.DEFAULT_BN_EPS if model_eps is None else float(model_eps)
    if snap_eps != model_eps:       # before anything is loaded: a refused snapshot leaves the model as it was
        raise ValueError("snapshot %s was written with batch-norm epsilon %g, the model runs %g (build it with bn_eps=%g)" %
                         (path, snap_eps, model_eps, snap_eps))
    if hasattr(model, "opts"):
        _v2snap.check_optimizer(path, adam is not None, snap_solver, getattr(model, "solver", None))
    _v2snap.check_matches("num_class", path, num_class, model.num_class)
    _v2snap.check_matches("anchors", path, anchors, np.asarray(model.anchors, np.float32).reshape(-1, 2))
    nets = model.networks()
    for s, net in zip(_v2snap.STACKS, nets):
        if len(stacks[s]) != net.num_layers:
            raise ValueError("snapshot %s: the %s stack has %d layers, the model has %d" %
                             (path, s, len(stacks[s]), net.num_layers))
        for l, layer in enumerate(stacks[s]):
            for k, shape in net._shapes(l).items():
                if tuple(layer[k].shape) != tuple(shape):
                    raise ValueError("snapshot %s: yolov2/%s/%d/%s has shape %s, the model expects %s" %
                                     (path, s, l, k, tuple(layer[k].shape), tuple(shape)))
        net.load_params(stacks[s])
    if hasattr(model, "opts") and (adam is not None or sgd is not None):
        for s, net, opt in zip(_v2snap.STACKS, nets, model.opts):
            if adam is not None:
                opt.load_state({"m": _layer_slots(net, adam[s]["m"]), "v": _layer_slots(net, adam[s]["v"]),
                                "t": adam[s]["t"]})
            else:
                opt.load_state({"accum": _layer_slots(net, sgd[s]["accum"]), "t": sgd[s]["t"]})
        sc = model.opts[0].scaler
        if sc is not None and scaler is not None:
            sc.ctrl.copy_(torch.as_tensor(scaler["ctrl"]))
            sc._apply(scaler["scale"])
            sc._clean = scaler["clean"]
            # the saved run read the control words one step late: the copy made after its last step is still to be looked
            # at by the next one
            sc._host.copy_(sc.ctrl)
            sc._event = torch.cuda.Event()
            sc._event.record()
    model.iteration = iteration
    return iteration


def read_yolov2_meta(path):
    """(anchors float32 [B][2], num_class, iteration) of a YOLOv2 snapshot, to build the model it restores into"""
    with np.load(path) as snap:
        return _v2snap.meta_from_blob(snap)


def read_yolov2_bn_eps(path):
    """the `bn_eps` argument of the model a YOLOv2 snapshot restores into: its yolov2/bn_eps, or None (the default)"""
    with np.load(path) as snap:
        eps = _v2snap.bn_eps_from_blob(snap)
    return None if eps == _v2snap.DEFAULT_BN_EPS else eps


def _is_darknet(model):
    """whether the model's graph is one a Darknet `.weights` file holds ("darknet", "tiny"): that file is its snapshot"""
    return getattr(model, "topology", "paper") in _yolov2.DARKNET_FILE_TOPOLOGIES


def _refuse_darknet_topology(model, what, instead):
    if _is_darknet(model):
        raise ValueError("%s: .npz snapshots of the \"%s\" topology are out of scope -- the .weights file is this "
                         "topology's snapshot (%s)" % (what, model.topology, instead))


def _ordered_snapshots(ckpt_dir, ext):
    """`train_iter_<i><ext>` files of ckpt_dir by iteration number, oldest first"""
    files = glob.glob(os.path.join(ckpt_dir, cfg.TRAIN_SNAPSHOT_PREFIX + "_iter_*" + ext))
    numbered = [(int(m.group(1)), f) for f in files for m in [re.search(r"_iter_(\d+)%s$" % re.escape(ext), f)] if m]
    return [f for _i, f in sorted(numbered)]


def get_ordered_yolov2_ckpts(ckpt_dir):
    """`train_iter_<i>.npz` files of ckpt_dir by iteration number, oldest first"""
    return _ordered_snapshots(ckpt_dir, ".npz")


def get_ordered_darknet_ckpts(ckpt_dir):
    """`train_iter_<i>.weights` files of ckpt_dir (the "darknet" topology's snapshots) by iteration number, oldest first"""
    return _ordered_snapshots(ckpt_dir, ".weights")


def read_darknet19_core(path):
    """the 18 core layers (dicts of the six arrays) of a Darknet-19 classifier or detector snapshot of this package
    (.npz or TF V2 checkpoint): what load_darknet19_backbone takes"""
    snap = _open_snapshot(path)
    names = _darknet.variable_names("classifier", 1000)[:len(engine.CORE_SPEC)]
    missing = [n for nm in names for n in nm.values() if n not in snap.files]
    if missing:
        raise ValueError("snapshot %s holds no Darknet-19 core: %s ... missing" % (path, missing[0]))
    return [{k: np.asarray(snap[n], np.float32) for k, n in nm.items()} for nm in names]


def load_darknet19_backbone(model, core_layers):
    """core_layers: the 18 conv-BN-leaky layers of Darknet-19 (a list of dicts W, b, gamma, beta, moving_mean,
    moving_var; longer lists -- a classifier's 19, a detector's 22 -- are cut) -> layers 0-12 into the stem and 13-17
    into the first five layers of the 13x13 stack of a YOLOv2Detector / YOLOv2Trainer; the two added 3x3 layers and the
    head keep their values.  Returns the number of layers loaded."""
    n_core = len(engine.CORE_SPEC)
    if len(core_layers) < n_core:
        raise ValueError("load_darknet19_backbone: %d layers given, the Darknet-19 core has %d" % (len(core_layers), n_core))
    stem, deep = model.networks()[:2]
    split = stem.num_layers
    for net, lo, hi in ((stem, 0, split), (deep, split, n_core)):
        layers = net.export_params()
        for l in range(lo, hi):
            for k, shape in net._shapes(l - lo).items():
                a = np.asarray(core_layers[l][k], np.float32)
                if tuple(a.shape) != tuple(shape):
                    raise ValueError("load_darknet19_backbone: core layer %d %s has shape %s, the model expects %s" %
                                     (l, k, tuple(a.shape), tuple(shape)))
                layers[l - lo][k] = a
        net.load_params(layers)
    return n_core


# ---------------------------------------------------------------------------
# Darknet's `.weights` files (utils/darknet_weights.py holds the format and the per-layer arithmetic, numpy only).
# load_darknet_weights / save_darknet_weights: a YOLOv2Detector(topology="darknet"), whose four stacks in networks()
# order are the file's convolutions in cfg order.  read_darknet_backbone: the 18 Darknet-19 layers of any such file
# (darknet19_448.conv.23) for the paper-topology trainer, through load_darknet19_backbone.  A YOLOv2DarknetTrainer has
# the same four stacks in networks() order and is taken wherever the detector is; load_darknet_prefix fills the leading
# layers of either from a shorter file, without a fold.
# ---------------------------------------------------------------------------
from ..utils import darknet_weights as _dkw
from . import yolov2 as _yolov2


def _darknet_model(model, what):
    if not _is_darknet(model):
        raise ValueError("%s takes a YOLOv2Detector(topology=\"darknet\" or \"tiny\") or a YOLOv2DarknetTrainer: the "
                         "paper topology's graph is not the one a Darknet file holds" % what)
    return model.networks()


def _file_layers(topology, specs):
    """[(k, c, n, batch_norm)] of the file of a Darknet graph from its stacks' specs, in networks() order: every layer
    with batch norm but the last; on "darknet" Darknet's filter size in the 18 core positions (its fourth layer is 1x1);
    on "tiny" the FILE's widths of the narrow layers (16 filters, and c = 16 behind them), which the stacks run padded"""
    topo = _yolov2._TOPOLOGY[topology]
    narrow = dict(topo.narrow)
    out = []
    for s, spec in enumerate(specs):
        for l, (k, ci, co, _pool) in enumerate(spec):
            if topology == "darknet" and len(out) < len(_dkw.DARKNET19_CORE):
                k = _dkw.DARKNET19_CORE[len(out)][0]
            if s == 0:
                ci, co = narrow.get(l - 1, ci), narrow.get(l, co)
            out.append((k, ci, co, not (s == len(specs) - 1 and l == len(spec) - 1)))
    return out


def darknet_file_layers(model):
    """[(k, c, n, batch_norm)] of the file a "darknet" or "tiny" detector or trainer reads and writes (_file_layers)"""
    nets = _darknet_model(model, "darknet_file_layers")
    if getattr(model, "cfg", None) is not None:          # a model built from a cfg: the file's own list
        return list(model.cfg.file_layers)
    return _file_layers(model.topology, [net.spec for net in nets])


def darknet_graph_floats(topology, num_class, num_anchors, width_div=1):
    """the float count of the `.weights` file of a Darknet graph at these classes, anchors and widths"""
    specs = _yolov2._TOPOLOGY[topology].specs(num_class, num_anchors, width_div)
    return sum(_dkw.layer_floats(l) for l in _file_layers(topology, specs))


def darknet_file_topology(path, num_class, num_anchors, width_div=1):
    """which Darknet graph a `.weights` file holds, by its float count -> "darknet" (yolov2-voc.cfg) or "tiny"
    (tiny-yolo-voc.cfg); a count that is neither raises, naming both expected counts"""
    values = _dkw.read(path)[4]
    counts = {t: darknet_graph_floats(t, num_class, num_anchors, width_div) for t in _yolov2.DARKNET_FILE_TOPOLOGIES}
    for t, n in counts.items():
        if n == values.size:
            return t
    raise ValueError("%s holds %d floats: at %d classes, %d anchors and width_div %d the \"darknet\" graph "
                     "(yolov2-voc.cfg) holds %d and the \"tiny\" graph (tiny-yolo-voc.cfg) holds %d" %
                     (path, values.size, num_class, num_anchors, width_div, counts["darknet"], counts["tiny"]))


def _other_graph(model):
    """for the float-count errors: what the file of the OTHER Darknet graph holds at the model's classes, anchors and width
    -- or, for a model built from a cfg, the cfg and its own count: no other graph is guessed"""
    if getattr(model, "cfg", None) is not None:
        return "the cfg %s describes %d floats" % (model.cfg.path, model.cfg.floats)
    (other,) = [t for t in _yolov2.DARKNET_FILE_TOPOLOGIES if t != model.topology]
    return "the \"%s\" graph at these classes, anchors and width_div %d holds %d floats" % (
        other, model.width_div, darknet_graph_floats(other, model.num_class, model.B, model.width_div))


def _describe(model):
    return "\"%s\" graph, %d classes, %d anchors, widths %s" % (model.topology, model.num_class, model.B,
                                                  "/".join(str(net.spec[-1][2]) for net in model.networks()))


def _load_darknet_layers(model, path, what, whole):
    """the one per-layer loop of load_darknet_weights (whole: the file must hold every convolution of the model) and
    load_darknet_prefix (its leading ones; the layers behind keep their values) -> (seen, layers read)"""
    nets = _darknet_model(model, what)
    file_layers = darknet_file_layers(model)
    _major, _minor, _revision, seen, values = _dkw.read(path)
    want = sum(_dkw.layer_floats(l) for l in file_layers)
    try:
        layers, _used = _dkw.split(values, file_layers)
    except ValueError as e:
        if whole:
            raise ValueError("%s holds %d floats, the model (%s: %d convolutions) needs %d; %s: %s" %
                             (path, values.size, _describe(model), len(file_layers), want, _other_graph(model), e))
        raise ValueError("%s holds %d floats, no whole-layer prefix of the model (%s: %d convolutions): %s" %
                         (path, values.size, _describe(model), len(file_layers), e))
    if whole and len(layers) != len(file_layers):
        raise ValueError("%s holds %d convolutions (%d floats), the model (%s) has %d (%d floats); %s" %
                         (path, len(layers), values.size, _describe(model), len(file_layers), want, _other_graph(model)))
    if not layers:
        raise ValueError("%s holds no convolution" % path)
    pos = 0
    for net in nets:
        take = min(net.num_layers, len(layers) - pos)
        if take <= 0:
            break
        params = net.export_params()
        for l in range(take):
            p = _dkw.to_layer_params(layers[pos + l], net.spec[l][0], model.bn_eps)
            p = _dkw.pad_layer_params(p, net.spec[l][1], net.spec[l][2])       # "tiny": the two narrow layers
            for k, shape in net._shapes(l).items():
                if tuple(p[k].shape) != tuple(shape):
                    raise ValueError("%s: convolution %d %s has shape %s, the model (%s) expects %s" %
                                     (path, pos + l, k, tuple(p[k].shape), _describe(model), tuple(shape)))
            params[l] = p
        net.load_params(params)
        pos += take
    wide = getattr(model, "wide", None)
    if wide is not None and pos == len(file_layers) - 1 and pos < len(layers):
        # the wide last layer (engine.WideHead): filters transposed as everywhere, b = the file's biases, no affine; packs
        d = layers[pos]
        wide.load(_dkw._filters_in(d["weights"], 1, np.float32), np.asarray(d["biases"], np.float32))
    if hasattr(model, "params_changed"):
        model.params_changed()      # a trainer's multi-scale contexts share the parameters just written: all re-pack
    return seen, len(layers)


def load_darknet_weights(model, path):
    """fill a YOLOv2Detector(topology="darknet") from a Darknet `.weights` file (yolov2-voc.weights) -> its `seen`.
    Per layer with batch norm: W = weights.transpose(2, 3, 1, 0) -- the first layer keeps Darknet's RGB order, the model
    feeds RGB --, b = 0, the four batch-norm arrays copied.  Last layer: b = biases and an inference batch norm that is
    the identity to one ulp (utils/darknet_weights.to_layer_params).  A file whose float count is not the one of the
    model's class count, anchors and width raises, naming both."""
    return _load_darknet_layers(model, path, "load_darknet_weights", True)[0]


def load_darknet_prefix(model, path):
    """the leading convolutions of a SHORTER Darknet file (darknet19_448.conv.23: the 18 core layers) into a
    "darknet"-topology model, detector or trainer -> the number of layers read.  The arithmetic of load_darknet_weights
    per layer and NO first-layer fold: this graph takes Darknet's input, so the import is exact on the border ring too
    (read_darknet_backbone, for the paper topology, is not).  The layers behind the prefix keep their values.  A file
    that ends inside a layer, holds more than the model or holds no layer at all raises."""
    return _load_darknet_layers(model, path, "load_darknet_prefix", False)[1]


def save_darknet_weights(model, path, seen, major=0, minor=1, revision=0):
    """the inverse, for a YOLOv2Detector(topology="darknet"): batch-norm layers with the conv bias folded into the mean,
    the last layer (it must run without activation: slope 1) with its inference affine folded into filters and biases
    (utils/darknet_weights.from_layer_params).  A model that load_darknet_weights filled and nothing changed gives the
    bytes that were read (write the header's version too: a file of version 0.2 has a 64-bit `seen`)."""
    nets = _darknet_model(model, "save_darknet_weights")
    wide = getattr(model, "wide", None)          # engine.WideHead: the file's last layer, behind an all-leaky head stack
    slopes = nets[-1].slopes                     # None: a context that was never given slopes runs 0.1 everywhere
    if wide is None and (slopes is None or float(slopes[-1]) != 1.0):
        raise ValueError("save_darknet_weights: the last layer runs with slope %s, Darknet's is linear (slope 1): its "
                         "batch norm cannot be folded through an activation" % (0.1 if slopes is None else slopes[-1]))
    file_layers = darknet_file_layers(model)
    out, pos = [], 0
    for net in nets:
        for l, p in enumerate(net.export_params()):
            kf, c, n, bn = file_layers[pos + l]
            out.append(_dkw.from_layer_params(_dkw.strip_layer_params(p, c, n), kf, bn, model.bn_eps))
        pos += net.num_layers
    if wide is not None:
        p = wide.export()
        out.append({"biases": p["b"], "weights": _dkw._filters_out(p["W"], 1, np.float32)})
    return _dkw.write(path, out, seen, major, minor, revision)


# ---------------------------------------------------------------------------
# One snapshot front for both topologies, keyed on model.topology / a topology name: the callers (pascal/) do not branch.
# "paper": train_iter_<i>.npz, the whole train state.  "darknet": train_iter_<i>.weights, parameters and `seen`.
# ---------------------------------------------------------------------------
_SNAPSHOT_EXT = {"paper": ".npz", "darknet": ".weights", "tiny": ".weights"}


def latest_yolov2_snapshot(ckpt_dir, topology):
    """the newest snapshot of `topology` in ckpt_dir, or None; a directory that holds snapshots of the OTHER format
    raises.  The two Darknet graphs share the .weights format: a file of the other one fails in the loader, by its
    float count"""
    other = [t for t in _SNAPSHOT_EXT if _SNAPSHOT_EXT[t] != _SNAPSHOT_EXT[topology]][0]    # .weights: named "darknet"
    foreign = _ordered_snapshots(ckpt_dir, _SNAPSHOT_EXT[other])
    if foreign:
        raise ValueError("--ckpt-dir %s holds snapshots of the %s topology (%s); this run trains the %s topology, whose "
                         "snapshots are %s files" % (ckpt_dir, other, os.path.basename(foreign[-1]), topology,
                                                     _SNAPSHOT_EXT[topology]))
    sfiles = _ordered_snapshots(ckpt_dir, _SNAPSHOT_EXT[topology])
    return sfiles[-1] if sfiles else None


def save_yolov2_snapshot(model, ckpt_dir, i):
    """snapshot `i` of a model into ckpt_dir, in its topology's format (`seen` = i * batch in a .weights file) -> the path"""
    path = os.path.join(ckpt_dir, cfg.TRAIN_SNAPSHOT_PREFIX + '_iter_' + str(i) +
                        _SNAPSHOT_EXT[getattr(model, "topology", "paper")])
    if _is_darknet(model):
        save_darknet_weights(model, path, seen=i * model.batch)
    else:
        save_yolov2_variables(model, path, iteration=i)
    return path


def restore_yolov2_snapshot(model, path):
    """a model from a snapshot of its topology -> the iteration it stood at.  A .weights file is the whole snapshot of the
    "darknet" topology: parameters, moving statistics and `seen`, no optimizer state -- the iteration is seen // batch,
    and a trainer continues there (resume_at)"""
    if not _is_darknet(model):
        return restore_yolov2_variables(model, path)
    iteration = load_darknet_weights(model, path) // model.batch
    if hasattr(model, "resume_at"):
        model.resume_at(iteration)
    return iteration


def read_darknet_backbone(path, bn_eps_model, width_div=1):
    """the 18 Darknet-19 core layers of a Darknet file (darknet19_448.conv.23, or the front of a longer one) as the dicts
    load_darknet19_backbone takes, for THIS repository's input convention -- uint8 BGR pixels mapped to [-1, 1), the
    paper-topology YOLOv2Trainer.  Per layer b = 0 and the batch-norm arrays are copied; Darknet's 1x1 fourth layer sits
    on the centre tap of this graph's 3x3 one.  The first layer's filter channels are reversed and halved and the
    constant sum(W) / 2 goes into moving_mean (utils/darknet_weights.fold_first_layer): exact in the interior, NOT on
    the one-pixel border ring of the first layer's output, where Darknet pads with black and this stack with mid-grey.
    Darknet's epsilon is 1e-6 and the variances are not bent to another one: a model on any other epsilon is refused.
    width_div: the narrow variant's widths (tests); a Darknet file carries no shapes."""
    if bn_eps_model is None or float(bn_eps_model) != _yolov2.DARKNET_BN_EPS:
        raise ValueError("read_darknet_backbone: the model's batch-norm epsilon is %s, Darknet's layers were trained with "
                         "%g -- build the trainer with YOLOv2Trainer(bn_eps=1e-6)" %
                         ("the default" if bn_eps_model is None else "%g" % float(bn_eps_model), _yolov2.DARKNET_BN_EPS))
    sa, sb, _sc = _yolov2.yolov2_specs(width_div=width_div)
    spec = (sa + sb)[:len(_dkw.DARKNET19_CORE)]
    file_layers = [(_dkw.DARKNET19_CORE[l][0], ci, co, True) for l, (_k, ci, co, _p) in enumerate(spec)]
    want = sum(_dkw.layer_floats(l) for l in file_layers)
    values = _dkw.read(path)[4]
    if values.size < want:
        raise ValueError("%s holds %d floats, the Darknet-19 core at width_div %d needs %d" %
                         (path, values.size, width_div, want))
    layers, _used = _dkw.split(values[:want], file_layers)
    out = [_dkw.to_layer_params(d, spec[l][0], bn_eps_model) for l, d in enumerate(layers)]
    out[0] = _dkw.fold_first_layer(out[0])
    return out
