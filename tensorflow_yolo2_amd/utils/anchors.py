"""Anchor shapes for the YOLOv2 head by dimension clustering (YOLO9000, section 2 "Dimension Clusters"): k-means over
the (width, height) of the training boxes with d(box, centroid) = 1 - IoU of the two shapes laid corner to corner, so
that the error does not grow with the box size as it does under the Euclidean distance.  Not in the reference (its head
has no anchors).  numpy, host only, deterministic: about 15 k boxes for VOC07 trainval."""
import numpy as np


def shape_iou(wh, centroids):
    """IoU of shapes that share a corner: wh [n][2], centroids [k][2] -> [n][k] float64"""
    wh = np.asarray(wh, np.float64).reshape(-1, 1, 2)
    c = np.asarray(centroids, np.float64).reshape(1, -1, 2)
    inter = np.minimum(wh[..., 0], c[..., 0]) * np.minimum(wh[..., 1], c[..., 1])
    return inter / (wh[..., 0] * wh[..., 1] + c[..., 0] * c[..., 1] - inter)


def kmeans_anchors(wh, k=5, seed=0, iters=100):
    """wh [n][2] positive (width, height) pairs -> float32 [k][2] centroids in the same unit, sorted by area.
    Start: one box drawn with `seed`, then k - 1 times the box farthest from the starts so far (the smallest best shape
    IoU; ties: the lowest index), which puts one start into every well-separated group; a step assigns every box to the
    centroid of the largest shape IoU (ties: the lowest index) and moves every centroid to the mean of its boxes (a
    centroid without boxes stays); it stops when no assignment changes, or after `iters` steps."""
    wh = np.asarray(wh, np.float64).reshape(-1, 2)
    if not (np.isfinite(wh).all() and (wh > 0).all()):
        raise ValueError("kmeans_anchors: widths and heights must be positive and finite")
    distinct = np.unique(wh, axis=0)
    if len(distinct) < k:
        raise ValueError("kmeans_anchors: %d distinct shapes for k = %d" % (len(distinct), k))
    rng = np.random.default_rng(seed)
    centroids = distinct[[int(rng.integers(0, len(distinct)))]]
    while len(centroids) < k:
        far = int(shape_iou(distinct, centroids).max(axis=1).argmin())
        centroids = np.concatenate([centroids, distinct[[far]]], axis=0)
    assign = np.full(len(wh), -1)
    for _ in range(int(iters)):
        nearest = shape_iou(wh, centroids).argmax(axis=1)
        if (nearest == assign).all():
            break
        assign = nearest
        for c in range(k):
            if (assign == c).any():
                centroids[c] = wh[assign == c].mean(axis=0)
    order = np.lexsort((centroids[:, 0], centroids[:, 0] * centroids[:, 1]))      # by area, then by width
    return centroids[order].astype(np.float32)


def mean_shape_iou(wh, anchors):
    """the clustering's figure of merit: mean over the boxes of the best shape IoU with an anchor"""
    return float(shape_iou(wh, anchors).max(axis=1).mean())


def box_table_wh(boxes, counts, table, size, entries=None):
    """(width, height) of every object of a DeviceVOC box table, in cells of stride 32 of the image stretched to
    size x size: boxes float64 [E][max_obj][5] = xmin, ymin, xmax, ymax, class; counts [E]; table int64 [E][5] = offset,
    height, width, pitch, flip (numpy arrays or tensors).  entries: the first that many rows (the mirrored copies of a
    flipped pool repeat the shapes).  Objects without extent are left out."""
    boxes, counts, table = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (boxes, counts, table))
    n = len(table) if entries is None else int(entries)
    out = []
    for e in range(n):
        h, w = float(table[e, 1]), float(table[e, 2])
        b = boxes[e, :int(counts[e]), :4].astype(np.float64)
        out.append(np.stack([(b[:, 2] - b[:, 0]) / w, (b[:, 3] - b[:, 1]) / h], axis=1) * (size / 32.0))
    wh = np.concatenate(out, axis=0) if out else np.zeros((0, 2))
    return wh[(wh > 0).all(axis=1)]
