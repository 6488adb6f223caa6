"""Batched evaluation of the detectors: the host specification of csrc/detect.hip (numpy only).

NOT in the reference (it has no evaluation code; SURVEY 8 a-x2).  Three functions, the per-image two of which the
kernels y2_detect_grid_batch and y2_voc_match_batch reproduce bit for bit, as img_dataset/augment.py is the
specification of csrc/augment.hip:

  grid_detect     one image's head output -> boxes in the 1-based pixels of the ORIGINAL image, after a score-ordered,
                  class-aware greedy NMS.  The decode is show_yolo_detection's (oracle/loss_ref.decode_detections,
                  csrc/loss.hip: decode_kernel) and the box is utils/voc_eval.detections_from_decode's.
  anchor_detect   the same rows for the YOLOv2 anchor head, from the outputs of y2_decode_anchors + y2_class_argmax
                  (kernel: y2_detect_anchor_batch, which decodes the raw head itself); shares grid_detect's walk.
  anchor_detect_classes  one row per (candidate, class) from y2_decode_anchors' scores [K][C]: anchor_detect per class
                  (kernel: y2_detect_anchor_classes_batch); class_rows flattens a batch of them for map_from_flags.
                  Both take net_size=N for a letterboxed input (img_dataset/pascal_voc.letterbox_u8): the boxes are
                  un-mapped from the picture's rectangle (kernels: y2_detect_anchor_batch_lb, ..._classes_batch_lb).
  anchor_detect_tree_darknet  Darknet's float rows for a word-tree head, one class (the node) per candidate: flat rows
                  under a class-aware walk (kernel: y2_detect_anchor_tree_batch_dk); the integer rows of such a head are
                  anchor_detect(boxes, objectness, node, ...) as it stands (kernel: y2_detect_anchor_tree_batch).
  match_image     the body of utils/voc_eval.eval_class for one image: a TP / FP / ignored flag per detection.
  map_from_flags  the global part: per class a stable sort by score, cumulative sums, utils/voc_eval.average_precision.

The split works because the devkit's matching is independent per image: a ground-truth box and its `taken` bit belong
to one image, so the flag of a detection depends only on the detections of its own image and class that rank before
it.  grid_detect returns an image's rows in descending score, which is the order eval_class meets them in; then
map_from_flags(rows of all images in image order) equals voc_eval.voc_map of the same detections, as floats.

Preconditions shared with the kernels (outside them the two sides may differ): the class values of a cell are not NaN
(the kernel's strict `>` walk skips a NaN, np.argmax returns it) and the box table holds finite boxes."""
import numpy as np

from . import voc_eval

LIMIT = float(1 << 30)     # a decoded product at or beyond it (or not finite) drops the candidate before any int()


def grid_candidates(predict, im_w, im_h, num_class, B, object_thresh):
    """every candidate of one image, before the ordering and the NMS:
    (valid bool [K], box int64 [K][4] = 1-based xmin, ymin, xmax, ymax (zero where not valid), cls int64 [K],
    score float32 [K]), K = S * S * B, candidate i = cell * B + b, cell = row * S + column"""
    predict = np.asarray(predict, np.float32)
    S = predict.shape[0]
    assert predict.shape == (S, S, num_class + 5 * B), predict.shape
    im_w, im_h = int(im_w), int(im_h)
    cells = predict.reshape(S * S, num_class + 5 * B)
    K = S * S * B
    cell = np.arange(K) // B
    b = np.arange(K) % B
    row, col = cell // S, cell % S
    score = cells[cell, num_class + b]                                    # float32
    pb = cells[:, num_class + B:].reshape(S * S, B, 4)[cell, b]           # float32 [K][4]
    with np.errstate(all="ignore"):
        dx = (pb[:, 0].astype(np.float64) + col) / float(S) * im_w
        dy = (pb[:, 1].astype(np.float64) + row) / float(S) * im_h
        dw = np.square(pb[:, 2]).astype(np.float64) * im_w                # np.square on float32, the product in float64
        dh = np.square(pb[:, 3]).astype(np.float64) * im_h
        prod = np.stack([dx, dy, dw, dh], axis=1)
        valid = score > np.float32(object_thresh)                         # (a NaN confidence compares false)
        valid &= (np.isfinite(prod) & (np.abs(prod) < LIMIT)).all(axis=1)
    prod = np.where(valid[:, None], prod, 0.0)
    x, y, w, h = (np.trunc(prod[:, k]).astype(np.int64) for k in range(4))   # int(): toward zero
    ulx, uly = x - w // 2, y - h // 2
    xmin, ymin = np.maximum(ulx, 0), np.maximum(uly, 0)                   # the box cut to the image: 0 .. im_w - 1
    xmax, ymax = np.minimum(ulx + w - 1, im_w - 1), np.minimum(uly + h - 1, im_h - 1)
    valid &= (xmax >= xmin) & (ymax >= ymin)
    box = np.stack([xmin, ymin, xmax, ymax], axis=1) + 1                  # the annotation's pixels are 1-based
    box = np.where(valid[:, None], box, 0)
    first = cells[:, :num_class]
    with np.errstate(all="ignore"):
        cls = np.where(np.isnan(first[:, 0]), 0, np.argmax(np.where(np.isnan(first), -np.inf, first), axis=1))[cell]
    return valid, box, cls.astype(np.int64), score


def grid_detect(predict, im_w, im_h, num_class, B, object_thresh, iou_thresh, max_out):
    """predict float32 [S][S][num_class + 5 B] of ONE image -> (det int32 [count][6] = xmin, ymin, xmax, ymax, class,
    candidate index; score float32 [count]), count <= max_out, rows in descending score (ties: ascending index)"""
    valid, box, cls, score = grid_candidates(predict, im_w, im_h, num_class, B, object_thresh)
    return _greedy_walk(valid, box, cls, score, iou_thresh, max_out)


def _greedy_walk(valid, box, cls, score, iou_thresh, max_out):
    """the ordering and the class-aware greedy NMS both detectors share: the valid candidates in descending score (ties:
    ascending index); a kept box suppresses every later box of its class with IoU (float64, + 1 extents) > iou_thresh;
    the walk stops at max_out kept rows -> (det int32 [count][6], score float32 [count])"""
    idx = np.nonzero(valid)[0]
    order = idx[np.lexsort((idx, -score[idx].astype(np.float64)))]        # score descending, then index ascending
    thresh = float(np.float32(iou_thresh))                                # the C ABI passes float
    suppressed = np.zeros(order.size, bool)
    keep = []
    for k in range(order.size):
        if len(keep) >= max_out:
            break
        if suppressed[k]:
            continue
        i = order[k]
        keep.append(i)
        later = order[k + 1:]
        if later.size:
            with np.errstate(all="ignore"):
                iou = voc_eval.box_iou_voc(box[i], box[later])
            suppressed[k + 1:] |= (cls[later] == cls[i]) & (iou > thresh)
    keep = np.asarray(keep, np.int64)
    det = np.concatenate([box[keep], cls[keep, None], keep[:, None]], axis=1).astype(np.int32).reshape(-1, 6)
    return det, score[keep].astype(np.float32)


def anchor_candidates(boxes, best, cls, im_w, im_h, score_thresh, net_size=None):
    """every candidate of one image of the YOLOv2 anchor head, from its decode: boxes float32 [K][4] = cx, cy, w, h
    relative to the image (what y2_decode_anchors writes), best float32 [K] and cls int [K] (what y2_class_argmax writes),
    candidate i = cell * B + b -> (valid, box, cls, score) as grid_candidates.  net_size None: the resize was a plain
    stretch, so the relative coordinates map straight to the original image: the float64 products cx * im_w, cy * im_h,
    w * im_w, h * im_h.  net_size N: the input was letterboxed (img_dataset/pascal_voc.letterbox_u8 at N) and the
    products are the exact inverse of that embedding, with (new_w, new_h, ox, oy) = letterbox_geometry(im_h, im_w, N):
    sx = im_w / new_w, sy = im_h / new_h, (cx * N - ox) * sx, (cy * N - oy) * sy, (w * N) * sx, (h * N) * sy in float64
    and in this order of operations.  From there on every rule is grid_candidates': a box that lies in a bar maps
    outside the image and comes out cut, or empty and dropped"""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    score = np.asarray(best, np.float32).reshape(-1)
    cls = np.asarray(cls).reshape(-1).astype(np.int64)
    assert len(boxes) == len(score) == len(cls), (boxes.shape, score.shape, cls.shape)
    im_w, im_h = int(im_w), int(im_h)
    with np.errstate(all="ignore"):
        if net_size is None:
            prod = boxes.astype(np.float64) * np.array([im_w, im_h, im_w, im_h], np.float64)
        else:
            prod = _letterbox_products(boxes, im_w, im_h, net_size)
        valid = score > np.float32(score_thresh)                          # (a NaN score compares false)
        valid &= (np.isfinite(prod) & (np.abs(prod) < LIMIT)).all(axis=1)
    prod = np.where(valid[:, None], prod, 0.0)
    x, y, w, h = (np.trunc(prod[:, k]).astype(np.int64) for k in range(4))   # int(): toward zero
    ulx, uly = x - w // 2, y - h // 2
    xmin, ymin = np.maximum(ulx, 0), np.maximum(uly, 0)
    xmax, ymax = np.minimum(ulx + w - 1, im_w - 1), np.minimum(uly + h - 1, im_h - 1)
    valid &= (xmax >= xmin) & (ymax >= ymin)
    box = np.stack([xmin, ymin, xmax, ymax], axis=1) + 1
    box = np.where(valid[:, None], box, 0)
    return valid, box, cls, score


def _letterbox_products(boxes, im_w, im_h, net_size):
    """float64 [K][4]: relative boxes of a letterboxed input of net_size -> x, y, w, h in pixels of the original image"""
    from ..img_dataset.pascal_voc import letterbox_geometry
    if int(net_size) != net_size or net_size < 32 or net_size % 32:
        raise ValueError("net_size %r is not a positive multiple of 32" % (net_size,))
    new_w, new_h, ox, oy = letterbox_geometry(im_h, im_w, net_size)
    n = np.float64(net_size)
    sx, sy = np.float64(im_w) / np.float64(new_w), np.float64(im_h) / np.float64(new_h)
    b = boxes.astype(np.float64)
    return np.stack([(b[:, 0] * n - np.float64(ox)) * sx, (b[:, 1] * n - np.float64(oy)) * sy,
                     (b[:, 2] * n) * sx, (b[:, 3] * n) * sy], axis=1)


def anchor_detect(boxes, best, cls, im_w, im_h, score_thresh, iou_thresh, max_out, net_size=None):
    """the decode of ONE image (anchor_candidates' arguments) -> grid_detect's rows: (det int32 [count][6] = xmin, ymin,
    xmax, ymax, class, candidate index; score float32 [count]); the specification of y2_detect_anchor_batch and, with
    net_size, of y2_detect_anchor_batch_lb"""
    valid, box, cls, score = anchor_candidates(boxes, best, cls, im_w, im_h, score_thresh, net_size=net_size)
    return _greedy_walk(valid, box, cls, score, iou_thresh, max_out)


def anchor_detect_classes(boxes, scores, im_w, im_h, score_thresh, iou_thresh, max_per_class, net_size=None):
    """one row per (candidate, class), as Darknet's `valid` writes them: boxes float32 [K][4] and scores float32 [K][C]
    of ONE image (what y2_decode_anchors writes) -> (det int32 [C][max_per_class][6], unused rows -1; score float32
    [C][max_per_class], unused 0; count int32 [C]).  Class c's rows are anchor_detect's with every candidate given the
    class c and the score scores[:, c]: a candidate is valid in every class whose score passes, and each class is
    ordered and walked on its own.  Column 4 is c, column 5 the candidate; the specification of
    y2_detect_anchor_classes_batch and, with net_size (anchor_candidates), of y2_detect_anchor_classes_batch_lb"""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    scores = np.asarray(scores, np.float32)
    scores = scores.reshape(len(boxes), -1)
    K, C = scores.shape
    det = np.full((C, max_per_class, 6), -1, np.int32)
    score = np.zeros((C, max_per_class), np.float32)
    count = np.zeros(C, np.int32)
    for c in range(C):
        d, s = anchor_detect(boxes, scores[:, c], np.full(K, c), im_w, im_h, score_thresh, iou_thresh, max_per_class,
                             net_size=net_size)
        count[c] = len(d)
        det[c, :len(d)] = d
        score[c, :len(d)] = s
    return det, score, count


# ---- Darknet's test-time protocol: float un-map, float centre-box NMS, float corners.  The specification
#      of csrc/darknet_io.hip; float32 in this operation order, double where it says so.
def darknet_unmap(boxes, im_w, im_h, net_size):
    """Darknet's correct_region_boxes for a letterboxed input: boxes float32 [K][4] = cx, cy, w, h relative to the
    net_size canvas -> float32 [K][4] = bx, by, bw, bh in pixels of the original image.  With new_w, new_h of
    letterbox_geometry: bx = float((double(cx) - double(N - new_w) / 2. / double(N)) / double(float(new_w) / float(N))),
    bw = w * (float(N) / float(new_w)), then bx * float(im_w), bw * float(im_w); y likewise.  The half offset is NOT
    rounded to the pixel the picture was embedded at: that is Darknet's"""
    from ..img_dataset.pascal_voc import letterbox_geometry
    if int(net_size) != net_size or net_size < 32 or net_size % 32:
        raise ValueError("net_size %r is not a positive multiple of 32" % (net_size,))
    f, d = np.float32, np.float64
    boxes = np.asarray(boxes, f).reshape(-1, 4)
    im_w, im_h, n = int(im_w), int(im_h), int(net_size)
    new_w, new_h, _, _ = letterbox_geometry(im_h, im_w, n)
    out = np.empty_like(boxes)
    with np.errstate(all="ignore"):
        for k, (new, im) in enumerate(((new_w, im_w), (new_h, im_h))):
            off = d(n - new) / d(2.0) / d(n)
            sc = d(f(new) / f(n))
            centre = ((boxes[:, k].astype(d) - off) / sc).astype(f)
            extent = boxes[:, 2 + k] * (f(n) / f(new))
            out[:, k] = centre * f(im)
            out[:, 2 + k] = extent * f(im)
    return out


def box_iou_darknet(a, b):
    """Darknet's box_iou on centre boxes (x, y, w, h), all float32: a [4], b [..., 4] -> float32 [...].
    overlap = min(x1 + w1 / 2, x2 + w2 / 2) - max(x1 - w1 / 2, x2 - w2 / 2) per axis; a negative overlap on either axis
    is no intersection; union = (aw * ah + bw * bh) - inter.  A zero union gives NaN, which compares false"""
    f = np.float32
    a = np.asarray(a, f)
    b = np.asarray(b, f)
    two = f(2.0)
    with np.errstate(all="ignore"):
        def overlap(x1, w1, x2, w2):
            return np.minimum(x1 + w1 / two, x2 + w2 / two) - np.maximum(x1 - w1 / two, x2 - w2 / two)
        ow = overlap(a[0], a[2], b[..., 0], b[..., 2])
        oh = overlap(a[1], a[3], b[..., 1], b[..., 3])
        inter = np.where((ow < 0) | (oh < 0), f(0.0), ow * oh).astype(f)
        union = (a[2] * a[3] + b[..., 2] * b[..., 3]) - inter
        return (inter / union).astype(f)


def darknet_corners(box, im_w, im_h):
    """centre boxes float32 [k][4] in pixels -> the row's float32 [k][4] = xmin, ymin, xmax, ymax as Darknet's `valid`
    prints them: float(double(bx) -/+ double(bw) / 2. + 1.), a minimum below 1 raised to 1, a maximum above the image
    size lowered to it"""
    f, d = np.float32, np.float64
    b = np.asarray(box, f).reshape(-1, 4).astype(d)
    with np.errstate(all="ignore"):
        xmin = (b[:, 0] - b[:, 2] / 2.0 + 1.0).astype(f)
        ymin = (b[:, 1] - b[:, 3] / 2.0 + 1.0).astype(f)
        xmax = (b[:, 0] + b[:, 2] / 2.0 + 1.0).astype(f)
        ymax = (b[:, 1] + b[:, 3] / 2.0 + 1.0).astype(f)
    xmin = np.where(xmin < f(1.0), f(1.0), xmin)
    ymin = np.where(ymin < f(1.0), f(1.0), ymin)
    xmax = np.where(xmax > f(im_w), f(im_w), xmax)
    ymax = np.where(ymax > f(im_h), f(im_h), ymax)
    return np.stack([xmin, ymin, xmax, ymax], axis=1).astype(f)


def anchor_detect_classes_darknet(boxes, scores, im_w, im_h, score_thresh, iou_thresh, max_per_class, net_size):
    """anchor_detect_classes under Darknet's protocol: boxes float32 [K][4] and scores float32 [K][C] of ONE image (what
    y2_decode_anchors writes) -> (det int32 [C][max_per_class][6], score float32 [C][max_per_class], count int32 [C]).
    Words 0..3 of a det row are the BIT PATTERNS of the float32 corners (det[..., :4].view(np.float32)), word 4 the
    class, word 5 the candidate; unused rows -1, unused scores 0.  A candidate is valid in class c if scores[:, c] >
    score_thresh (NaN compares false) and its four darknet_unmap values are finite -- no other rule: a box that is empty
    after the cut is kept.  Per class: descending score, ties by ascending candidate (our rule: qsort leaves ties open);
    a kept box suppresses every later one with box_iou_darknet > iou_thresh on the centre boxes; the walk stops at
    max_per_class rows (our cap).  The specification of y2_detect_anchor_classes_batch_dk"""
    f = np.float32
    boxes = np.asarray(boxes, f).reshape(-1, 4)
    scores = np.asarray(scores, f).reshape(len(boxes), -1)
    K, C = scores.shape
    px = darknet_unmap(boxes, im_w, im_h, net_size)
    finite = np.isfinite(px).all(axis=1)
    thresh = f(iou_thresh)
    det = np.full((C, max_per_class, 6), -1, np.int32)
    score = np.zeros((C, max_per_class), f)
    count = np.zeros(C, np.int32)
    for c in range(C):
        with np.errstate(all="ignore"):
            idx = np.nonzero((scores[:, c] > f(score_thresh)) & finite)[0]
        order = idx[np.lexsort((idx, -scores[idx, c].astype(np.float64)))]
        suppressed = np.zeros(order.size, bool)
        keep = []
        for k in range(order.size):
            if len(keep) >= max_per_class:
                break
            if suppressed[k]:
                continue
            keep.append(order[k])
            later = order[k + 1:]
            if later.size:
                suppressed[k + 1:] |= box_iou_darknet(px[order[k]], px[later]) > thresh
        keep = np.asarray(keep, np.int64)
        count[c] = len(keep)
        det[c, :len(keep), :4] = darknet_corners(px[keep], im_w, im_h).view(np.int32)
        det[c, :len(keep), 4] = c
        det[c, :len(keep), 5] = keep
        score[c, :len(keep)] = scores[keep, c]
    return det, score, count


def anchor_detect_tree_darknet(boxes, so, top, im_w, im_h, score_thresh, iou_thresh, max_out, net_size):
    """Darknet's rows for a word-tree head, where a candidate has ONE class: boxes float32 [K][4] and so float32 [K] of
    ONE image (what y2_decode_anchors writes: the box, the objectness), top int [K] the node of each candidate
    (utils/word_tree.word_tree_head) -> (det int32 [count][6], score float32 [count]), count <= max_out: FLAT rows in one
    descending order (ties by ascending candidate).  Words 0..3 of a row are the bit patterns of darknet_corners, word 4
    the node, word 5 the candidate.  A candidate is valid if so > score_thresh (NaN compares false), top >= 0 (the -1 of a
    row the walk skipped; the kernel, which knows the node count, drops a top at or beyond it too: pass -1 for those) and
    its four darknet_unmap values are finite -- no other rule.  The walk is class-aware: a kept box suppresses every later one of the SAME node with box_iou_darknet >
    iou_thresh, so the rows of node c are segment c of anchor_detect_classes_darknet on scores one-hot so at top, where no
    cap binds.  The integer-row counterpart is anchor_detect(boxes, so, top, ...).  The specification of
    y2_detect_anchor_tree_batch_dk"""
    f = np.float32
    boxes = np.asarray(boxes, f).reshape(-1, 4)
    so = np.asarray(so, f).reshape(-1)
    top = np.asarray(top).reshape(-1).astype(np.int64)
    assert len(boxes) == len(so) == len(top), (boxes.shape, so.shape, top.shape)
    px = darknet_unmap(boxes, im_w, im_h, net_size)
    thresh = f(iou_thresh)
    with np.errstate(all="ignore"):
        idx = np.nonzero((so > f(score_thresh)) & (top >= 0) & np.isfinite(px).all(axis=1))[0]
    order = idx[np.lexsort((idx, -so[idx].astype(np.float64)))]
    suppressed = np.zeros(order.size, bool)
    keep = []
    for k in range(order.size):
        if len(keep) >= max_out:
            break
        if suppressed[k]:
            continue
        keep.append(order[k])
        later = order[k + 1:]
        if later.size:
            suppressed[k + 1:] |= (top[later] == top[order[k]]) & (box_iou_darknet(px[order[k]], px[later]) > thresh)
    keep = np.asarray(keep, np.int64)
    det = np.empty((len(keep), 6), np.int32)
    det[:, :4] = darknet_corners(px[keep], im_w, im_h).view(np.int32)
    det[:, 4] = top[keep]
    det[:, 5] = keep
    return det, so[keep].astype(f)


def match_image_f(det, gt_boxes, gt_difficult, iou_thresh=0.5):
    """match_image for rows whose corners are float32: det [k][>= 5] = xmin, ymin, xmax, ymax (float32 values, or the
    int32 bit patterns of anchor_detect_classes_darknet's rows) and the class.  The rules are match_image's; the devkit's
    IoU (float64, + 1 extents) works on the four float32 values promoted to double, not on the six decimals a results
    file would keep.  The specification of y2_voc_match_batch_f"""
    det = np.asarray(det)
    det = det.reshape(-1, det.shape[-1]) if det.size else det.reshape(0, 6)
    if det.dtype == np.int32:
        corners = np.ascontiguousarray(det[:, :4]).view(np.float32)
    else:
        corners = det[:, :4].astype(np.float32)
    cls = det[:, 4]
    gt = np.asarray(gt_boxes, np.float64).reshape(-1, 5)
    difficult = np.asarray(gt_difficult).reshape(-1).astype(bool)
    taken = np.zeros(len(gt), bool)
    thresh = float(np.float32(iou_thresh))
    flags = np.zeros(len(det), np.int32)
    for k in range(len(det)):
        objs = np.nonzero(gt[:, 4] == float(cls[k]))[0]
        if not objs.size:
            continue
        with np.errstate(all="ignore"):
            ious = voc_eval.box_iou_voc(tuple(float(v) for v in corners[k]), gt[objs, :4])
        j = int(ious.argmax())                                            # first maximum, taken objects included
        if not float(ious[j]) >= thresh:
            continue
        j = objs[j]
        if difficult[j]:
            flags[k] = 2
        elif not taken[j]:
            flags[k] = 1
            taken[j] = True
    return flags


def class_rows(det, score, count, flags):
    """a batch of anchor_detect_classes outputs (det [n][C][M][6], score [n][C][M], count [n][C]) with the flags of
    match_image per (image, class) segment (flags [n][C][M]) -> the (class, score, flag) rows map_from_flags takes:
    image-major, then class, then rank"""
    det, score, count, flags = (np.asarray(a) for a in (det, score, count, flags))
    live = np.arange(det.shape[2])[None, None, :] < count[:, :, None]
    return det[live][:, 4], score[live], flags[live]


def match_image(det, gt_boxes, gt_difficult, iou_thresh=0.5):
    """det int [k][>= 5] = xmin, ymin, xmax, ymax, class in descending score; gt_boxes float64 [m][5] = xmin, ymin,
    xmax, ymax, class (a row of DeviceVOC's box table); gt_difficult [m] -> int32 [k]: 1 true positive, 0 false
    positive, 2 ignored (the object is difficult)"""
    det = np.asarray(det)
    det = det.reshape(-1, det.shape[-1]) if det.size else det.reshape(0, 6)
    gt = np.asarray(gt_boxes, np.float64).reshape(-1, 5)
    difficult = np.asarray(gt_difficult).reshape(-1).astype(bool)
    taken = np.zeros(len(gt), bool)
    thresh = float(np.float32(iou_thresh))
    flags = np.zeros(len(det), np.int32)
    for k, d in enumerate(det):
        objs = np.nonzero(gt[:, 4] == float(d[4]))[0]
        if not objs.size:
            continue
        with np.errstate(all="ignore"):
            ious = voc_eval.box_iou_voc((int(d[0]), int(d[1]), int(d[2]), int(d[3])), gt[objs, :4])
        j = int(ious.argmax())                                            # first maximum, taken objects included
        if not float(ious[j]) >= thresh:
            continue
        j = objs[j]
        if difficult[j]:
            flags[k] = 2
        elif not taken[j]:
            flags[k] = 1
            taken[j] = True
    return flags


def npos_from_objects(classes, difficult):
    """{class: number of non-difficult objects} over the classes that have ground truth at all (a class whose objects
    are all difficult is evaluated, with 0), from parallel sequences over every object of the image set"""
    npos = {}
    for c, d in zip(classes, difficult):
        npos[int(c)] = npos.get(int(c), 0) + (0 if d else 1)
    return npos


def map_from_flags(rows, npos, use_07_metric=True):
    """rows = (class [N], score [N], flag [N]) of the detections of all images IN IMAGE ORDER, each image's in
    match_image's order; npos: {class: non-difficult objects} with one key per class that has ground truth (or a
    sequence indexed by class: the classes with npos > 0) -> (mAP over those classes, {class: AP}), as
    voc_eval.voc_map"""
    cls, score, flag = (np.asarray(a).reshape(-1) for a in rows)
    if not isinstance(npos, dict):
        npos = {c: int(n) for c, n in enumerate(npos) if n > 0}
    eps = np.finfo(np.float64).eps
    aps = {}
    for c in sorted(npos):
        sel = (cls == c) & (flag != 2)
        order = np.argsort(-score[sel].astype(np.float64), kind="stable")
        f = flag[sel][order]
        ctp, cfp = np.cumsum((f == 1).astype(np.float64)), np.cumsum((f == 0).astype(np.float64))
        recall = ctp / max(npos[c], 1)
        precision = ctp / np.maximum(ctp + cfp, eps)
        aps[c] = voc_eval.average_precision(recall, precision, use_07_metric)
    return (float(np.mean(list(aps.values()))) if aps else 0.0), aps
