"""Region loss of the YOLOv2 anchor head on BOX LISTS, as a host specification (numpy only): the loss of
oracle/ext_ref.py yolov2_loss with every ground-truth box of an image kept (img_dataset/augment.encode_box_list), plus
the two terms of Darknet's region layer that the grid-label loss leaves out -- the (2 - w h) weight of the coordinate
terms and the anchor-prior term of the first images.  Not in the reference (its model is the grid detector); the kernel
y2_yolov2_loss_boxes (csrc/ext.hip) is tested against this file.

Per image, truth [T][5] = cx, cy, w, h in pixels of the resized input and the class index; the first ntruth rows count.
  cell units      g = t / image_size * S, in `dtype`
  cell of truth k q = min(int(gx), S - 1), r = min(int(gy), S - 1): derived here, not stored
  responsible     bs = the first maximum over the anchors of the shape IoU min(gw, aw) min(gh, ah) / (gw gh + aw ah - inter)
  owner           of slot (r, q, bs): the LOWEST truth index that claims it ("first wins").  A truth that loses its slot
                  has no coord / object / class term, but still counts in `best`
  best[r, q, b]   max over ALL truths of the image of the centre-form IoU with the decoded prediction
  owned slot      the coord, object and class terms of oracle/ext_ref.py yolov2_loss (IoU target held constant); with
                  area_weight the coord terms and their gradients times 2 - (gw / S) (gh / S)
  un-owned slot   noobject_scale * sig(to)^2 where best <= thresh; with prior_scale > 0 also
                  prior_scale * ((sig(tx) - 1/2)^2 + (sig(ty) - 1/2)^2 + tw^2 + th^2), counted in the coord part
  loss            parts / N in the order coord, object, noobject, class, then their sum"""
import numpy as np

YOLOV2_SCALES = dict(coord_scale=1.0, object_scale=5.0, noobject_scale=1.0, class_scale=1.0, thresh=0.6)


def _box_iou_cwh(ax, ay, aw, ah, bx, by, bw, bh):
    iw = np.maximum(0.0, np.minimum(ax + aw / 2, bx + bw / 2) - np.maximum(ax - aw / 2, bx - bw / 2))
    ih = np.maximum(0.0, np.minimum(ay + ah / 2, by + bh / 2) - np.maximum(ay - ah / 2, by - bh / 2))
    inter = iw * ih
    uni = aw * ah + bw * bh - inter
    return np.where(uni > 0, inter / np.where(uni > 0, uni, 1.0), 0.0)


def shape_ious(gw, gh, anchors):
    """shape IoU of a box of gw x gh cells with every anchor [B][2] (both centred on one point)"""
    inter = np.minimum(gw, anchors[:, 0]) * np.minimum(gh, anchors[:, 1])
    return inter / (gw * gh + anchors[:, 0] * anchors[:, 1] - inter)


def yolov2_loss_boxes(net, truth, ntruth, anchors, image_size, coord_scale=1.0, object_scale=5.0, noobject_scale=1.0,
                      class_scale=1.0, thresh=0.6, area_weight=False, prior_scale=0.0, dtype=np.float64,
                      return_margins=False):
    """-> (loss[5] = coord, object, noobject, class, total; dnet [N,S,S,B,5+C]); with return_margins a third value, the
    decision margins of this input: {"best_thresh": least |best - thresh| over all (cell, anchor) pairs, "shape_gap":
    least gap between the two best shape IoUs of a truth, "cell_edge": least distance (cell units) of a truth centre
    from a cell edge}; inf where there is nothing to decide.  A comparison against float32 arithmetic is meaningful only
    on inputs whose margins are well above float32 rounding."""
    net = np.asarray(net, dtype)
    truth = np.asarray(truth, dtype)
    ntruth = np.asarray(ntruth).astype(np.int64)
    an = np.asarray(anchors, dtype)
    n, s, _, b, d = net.shape
    c = d - 5
    assert truth.ndim == 3 and truth.shape[0] == n and truth.shape[2] == 5, truth.shape
    assert ntruth.shape == (n,) and (ntruth >= 0).all() and (ntruth <= truth.shape[1]).all(), ntruth
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    dnet = np.zeros_like(net)
    parts = np.zeros(4, dtype)
    col = np.arange(s, dtype=dtype)[None, :, None]
    row = np.arange(s, dtype=dtype)[:, None, None]
    margins = {"best_thresh": np.inf, "shape_gap": np.inf, "cell_edge": np.inf}
    for i in range(n):
        t = net[i]
        sx, sy, so = sig(t[..., 0]), sig(t[..., 1]), sig(t[..., 4])
        px, py = sx + col, sy + row
        pw, ph = an[None, None, :, 0] * np.exp(t[..., 2]), an[None, None, :, 1] * np.exp(t[..., 3])
        truths = []
        for k in range(int(ntruth[i])):
            tr = truth[i, k]
            gx, gy = tr[0] / image_size * s, tr[1] / image_size * s
            gw, gh = tr[2] / image_size * s, tr[3] / image_size * s
            truths.append((gx, gy, gw, gh, int(tr[4]), min(int(gy), s - 1), min(int(gx), s - 1)))
            for g in (gx, gy):
                frac = float(g) - np.floor(float(g))
                margins["cell_edge"] = min(margins["cell_edge"], frac, 1.0 - frac)
        best = np.zeros((s, s, b), dtype)
        for (gx, gy, gw, gh, _k, _r, _q) in truths:
            best = np.maximum(best, _box_iou_cwh(px, py, pw, ph, gx, gy, gw, gh))
        margins["best_thresh"] = min(margins["best_thresh"], float(np.abs(best - thresh).min()))
        owned = np.zeros((s, s, b), bool)
        for (gx, gy, gw, gh, k, r, q) in truths:
            shape_iou = shape_ious(gw, gh, an)
            bs = int(np.argmax(shape_iou))                       # first maximum
            if b > 1:
                two = np.sort(shape_iou)[-2:]
                margins["shape_gap"] = min(margins["shape_gap"], float(two[1] - two[0]))
            if owned[r, q, bs]:
                continue                                         # a lower truth index owns the slot
            owned[r, q, bs] = True
            tt = t[r, q, bs]
            wgt = coord_scale * ((2.0 - (gw / s) * (gh / s)) if area_weight else 1.0)
            ex, ey = sx[r, q, bs] - (gx - q), sy[r, q, bs] - (gy - r)
            ew, eh = tt[2] - np.log(gw / an[bs, 0]), tt[3] - np.log(gh / an[bs, 1])
            parts[0] += wgt * (ex * ex + ey * ey + ew * ew + eh * eh)
            dnet[i, r, q, bs, 0] = wgt * 2 * ex * sx[r, q, bs] * (1 - sx[r, q, bs])
            dnet[i, r, q, bs, 1] = wgt * 2 * ey * sy[r, q, bs] * (1 - sy[r, q, bs])
            dnet[i, r, q, bs, 2] = wgt * 2 * ew
            dnet[i, r, q, bs, 3] = wgt * 2 * eh
            iou = float(_box_iou_cwh(px[r, q, bs], py[r, q, bs], pw[r, q, bs], ph[r, q, bs], gx, gy, gw, gh))
            eo = so[r, q, bs] - iou
            parts[1] += object_scale * eo * eo
            dnet[i, r, q, bs, 4] = object_scale * 2 * eo * so[r, q, bs] * (1 - so[r, q, bs])
            if 0 <= k < c:                                       # (a class index outside [0, C) takes no class term)
                lg = tt[5:]
                m = lg.max()
                lse = m + np.log(np.exp(lg - m).sum())
                parts[3] += class_scale * (lse - lg[k])
                sm = np.exp(lg - lse)
                sm[k] -= 1.0
                dnet[i, r, q, bs, 5:] = class_scale * sm
        free = ~owned
        noobj = free & (best <= thresh)
        parts[2] += noobject_scale * (so[noobj] ** 2).sum()
        dnet[i, ..., 4] += np.where(noobj, noobject_scale * 2 * so * so * (1 - so), 0.0)
        if prior_scale > 0:
            tw, th = t[..., 2], t[..., 3]
            prior = (sx - 0.5) ** 2 + (sy - 0.5) ** 2 + tw * tw + th * th
            parts[0] += prior_scale * prior[free].sum()
            dnet[i, ..., 0] += np.where(free, prior_scale * 2 * (sx - 0.5) * sx * (1 - sx), 0.0)
            dnet[i, ..., 1] += np.where(free, prior_scale * 2 * (sy - 0.5) * sy * (1 - sy), 0.0)
            dnet[i, ..., 2] += np.where(free, prior_scale * 2 * tw, 0.0)
            dnet[i, ..., 3] += np.where(free, prior_scale * 2 * th, 0.0)
    parts = parts / n
    dnet = dnet / n
    loss = np.concatenate([parts, [parts.sum()]]).astype(dtype)
    return (loss, dnet, margins) if return_margins else (loss, dnet)


REGION_STATS = ("avg_iou", "class", "obj", "no_obj", "avg_recall", "count")
REGION_STATS_LINE = "Region Avg IOU: %f, Class: %f, Obj: %f, No Obj: %f, Avg Recall: %f,  count: %d"


def region_stats_boxes(net, truth, ntruth, anchors, image_size, dtype=np.float64, return_margins=False):
    """the numbers of Darknet's region-layer log line, from the inputs of yolov2_loss_boxes and with its derivations (cell
    units, the cell (r, q), the first-maximum shape-IoU anchor bs, the decoded prediction, the centre-form IoU).  EVERY
    listed truth counts, owner of its slot or not: Darknet's region layer has no ownership rule.  Per truth k: iou_k of
    the prediction at (r, q, bs) with the truth, obj_k = sig(to) there, cls_k = softmax(class logits)[class] there when
    0 <= class < C.  -> stats[6] = mean iou_k; mean cls_k over the truths with a valid class; mean obj_k; mean sig(to)
    over all N S S B slots; share of truths with iou_k > 0.5; the truth count.  A mean over nothing is 0 (Darknet prints
    NaN there).  With return_margins a second value: {"iou_half": least |iou_k - 0.5|, "shape_gap", "cell_edge"}, the
    last two as yolov2_loss_boxes defines them."""
    net = np.asarray(net, dtype)
    truth = np.asarray(truth, dtype)
    ntruth = np.asarray(ntruth).astype(np.int64)
    an = np.asarray(anchors, dtype)
    n, s, _, b, d = net.shape
    c = d - 5
    assert truth.ndim == 3 and truth.shape[0] == n and truth.shape[2] == 5, truth.shape
    assert ntruth.shape == (n,) and (ntruth >= 0).all() and (ntruth <= truth.shape[1]).all(), ntruth
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    margins = {"iou_half": np.inf, "shape_gap": np.inf, "cell_edge": np.inf}
    ious, objs, clss = [], [], []
    for i in range(n):
        for k in range(int(ntruth[i])):
            tr = truth[i, k]
            gx, gy = tr[0] / image_size * s, tr[1] / image_size * s
            gw, gh = tr[2] / image_size * s, tr[3] / image_size * s
            r, q = min(int(gy), s - 1), min(int(gx), s - 1)
            for g in (gx, gy):
                frac = float(g) - np.floor(float(g))
                margins["cell_edge"] = min(margins["cell_edge"], frac, 1.0 - frac)
            shape_iou = shape_ious(gw, gh, an)
            bs = int(np.argmax(shape_iou))                       # first maximum
            if b > 1:
                two = np.sort(shape_iou)[-2:]
                margins["shape_gap"] = min(margins["shape_gap"], float(two[1] - two[0]))
            t = net[i, r, q, bs]
            iou = float(_box_iou_cwh(sig(t[0]) + q, sig(t[1]) + r, an[bs, 0] * np.exp(t[2]), an[bs, 1] * np.exp(t[3]),
                                     gx, gy, gw, gh))
            margins["iou_half"] = min(margins["iou_half"], abs(iou - 0.5))
            ious.append(iou)
            objs.append(sig(t[4]))
            cls = int(tr[4])
            if 0 <= cls < c:
                lg = t[5:]
                m = lg.max()
                clss.append(np.exp(lg[cls] - m) / np.exp(lg - m).sum())
    mean = lambda v: float(np.mean(np.asarray(v, dtype))) if len(v) else 0.0
    stats = np.array([mean(ious), mean(clss), mean(objs), float(sig(net[..., 4]).mean()),
                      mean([float(v > 0.5) for v in ious]), float(len(ious))], dtype)
    return (stats, margins) if return_margins else stats


def grid_to_box_list(labels, max_boxes=None):
    """the box list of a label grid [N,S,S,5+C] (one object per cell): its occupied cells in row-major order ->
    (truth [N][T][5] float32, ntruth [N] int32), T = max_boxes or the largest count (at least 1)"""
    labels = np.asarray(labels)
    n = labels.shape[0]
    rows = [[(*lab[1:5], float(np.argmax(lab[5:]))) for lab in labels[i][labels[i, :, :, 0] > 0]] for i in range(n)]
    t = max_boxes or max(1, max(len(r) for r in rows))
    truth = np.zeros((n, t, 5), np.float32)
    ntruth = np.zeros(n, np.int32)
    for i, r in enumerate(rows):
        r = r[:t]
        ntruth[i] = len(r)
        if r:
            truth[i, :len(r)] = np.asarray(r, np.float32)
    return truth, ntruth
