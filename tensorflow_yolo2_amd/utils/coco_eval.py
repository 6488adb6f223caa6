"""COCO's bounding-box evaluation on the host, in numpy float64: the specification of y2_coco_match_batch (csrc/coco.hip)
and everything around it -- the annotation reader, the accumulation into precision / recall arrays, the twelve summary
numbers and the results file Darknet's `valid` writes.  Not in the reference (it has no evaluation code).

This is a restatement of `COCOeval` with iouType="bbox", useCats=1, and of `bbIou` of the mask API.  Neither program nor
any COCO file was at hand when this was written: the rules are stated from memory of the two ("COCO
evaluation").  What is checked is that the device equals this file bit for bit and that this file equals a second,
literal restatement of `evaluateImg`'s sorted loop (tests/test_coco_eval_host.py).

Rows.  A detection row is six int32 words as the detect kernels write them; columns 0..3 are corners, column 4 is the
class.  row_form 0: the integer rows of y2_detect_anchor_classes_batch[_lb], 1-based inclusive corners.  row_form 1: the
float rows of y2_detect_anchor_classes_batch_dk, words 0..3 the bit patterns of float32 corners that both carry
Darknet's + 1.  row_xywh turns either into COCO's x, y, w, h (zero-based continuous corner, no + 1 extent).

The `rows` of accumulate and write_results is a dict of parallel arrays in SEGMENT order -- image (entry) ascending, then
class, every (image, class) segment in descending score, the order the evaluation buffer has:
    "image" [R] entry index into dataset["images"], "class" [R] category index, "score" [R],
    "match" [R][A] the packed words of match_segment, "bbox" [R][4] x, y, w, h of row_xywh.
The `dataset` is read_instances' dict."""
import json
import os

import numpy as np

THRESHOLDS = np.linspace(0.5, 0.95, 10)
AREA_RANGES = np.array([[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]], np.float64)   # all, small, medium, large
MAX_DETS = (1, 10, 100)
MAX_THRESHOLDS, MAX_AREAS = 16, 4                 # Y2_COCO_MAX_THRESHOLDS, Y2_COCO_MAX_AREAS; and T * A <= 64
RECALL_POINTS = 101


def bbox_iou(d, g, crowd):
    """IoU of two x, y, w, h boxes (bbIou): every operation a separate double operation, in this order.  With `crowd`
    the union is the detection's own area: a detection inside a crowd region overlaps it fully"""
    dx, dy, dw, dh = (np.float64(v) for v in d[:4])
    gx, gy, gw, gh = (np.float64(v) for v in g[:4])
    da = dw * dh
    ga = gw * gh
    ow = min(dx + dw, gx + gw) - max(dx, gx)
    if ow <= 0:
        return np.float64(0.0)
    oh = min(dy + dh, gy + gh) - max(dy, gy)
    if oh <= 0:
        return np.float64(0.0)
    i = ow * oh
    u = da if crowd else (da + ga) - i
    with np.errstate(all="ignore"):
        return i / u


def _rows(rows):
    """int32 [r][words]; no rows: [0][6]"""
    rows = np.asarray(rows, np.int32)
    return rows.reshape(len(rows), -1) if rows.size else np.zeros((0, 6), np.int32)


def row_xywh(rows, row_form):
    """int32 rows [r][>= 4] -> float64 [r][4] = x, y, w, h in COCO's convention"""
    rows = _rows(rows)
    if row_form == 0:
        c = rows[:, :4].astype(np.float64)
        return np.stack([c[:, 0] - 1.0, c[:, 1] - 1.0, c[:, 2] - c[:, 0] + 1.0, c[:, 3] - c[:, 1] + 1.0], axis=1)
    if row_form == 1:
        c = np.ascontiguousarray(rows[:, :4]).view(np.float32).astype(np.float64)
        return np.stack([c[:, 0] - 1.0, c[:, 1] - 1.0, c[:, 2] - c[:, 0], c[:, 3] - c[:, 1]], axis=1)
    raise ValueError("row_form %r is neither 0 (integer rows) nor 1 (float rows)" % (row_form,))


def _limits(thresholds, area_ranges):
    thresholds = np.asarray(THRESHOLDS if thresholds is None else thresholds, np.float64).reshape(-1)
    area_ranges = np.asarray(AREA_RANGES if area_ranges is None else area_ranges, np.float64).reshape(-1, 2)
    T, A = len(thresholds), len(area_ranges)
    if not (1 <= T <= MAX_THRESHOLDS and 1 <= A <= MAX_AREAS and T * A <= 64):
        raise ValueError("%d thresholds and %d area ranges: at most %d and %d, and at most 64 pairs"
                         % (T, A, MAX_THRESHOLDS, MAX_AREAS))
    return thresholds, area_ranges


def match_segment(rows, gt, area, crowd, thresholds=None, area_ranges=None, row_form=0):
    """rows int32 [r][>= 5] of ONE segment in their given order (descending score); gt float64 [m][5] = x, y, w, h, class
    of the image's annotations in file order, area [m] (the annotation's `area` field, not w * h), crowd [m] ->
    int32 [r][A]: bits 2t, 2t + 1 of word a hold 1 (true positive), 0 (false positive) or 2 (ignored) under threshold t
    and area range a.  The two passes are evaluateImg's loop over ground truths sorted non-ignored first, with its break"""
    thresholds, area_ranges = _limits(thresholds, area_ranges)
    rows = _rows(rows)
    gt = np.asarray(gt, np.float64).reshape(-1, 5)
    area = np.asarray(area, np.float64).reshape(-1)
    crowd = np.asarray(crowd).reshape(-1).astype(bool)
    box = row_xywh(rows, row_form)
    out = np.zeros((len(rows), len(area_ranges)), np.uint32)     # bit 31 is threshold 15's
    # the IoUs do not depend on (a, t): once per (row, ground truth of the row's class)
    ious = [{j: bbox_iou(box[r], gt[j], crowd[j]) for j in range(len(gt)) if gt[j, 4] == rows[r, 4]}
            for r in range(len(rows))]
    for a, (lo, hi) in enumerate(area_ranges):
        ignored = crowd | (area < lo) | (area > hi)
        for t, thr in enumerate(thresholds):
            matched = np.zeros(len(gt), bool)
            for r in range(len(rows)):
                best, m = min(thr, 1 - 1e-10), None
                for j in ious[r]:                                   # first pass: the non-ignored, annotation order
                    if ignored[j] or matched[j] or ious[r][j] < best:
                        continue
                    best, m = ious[r][j], j
                if m is None:
                    for j in ious[r]:                               # second pass: the ignored
                        if not ignored[j] or (matched[j] and not crowd[j]) or ious[r][j] < best:
                            continue
                        best, m = ious[r][j], j
                if m is not None:
                    matched[m] = True
                    value = 2 if ignored[m] else 1
                else:
                    own = box[r, 2] * box[r, 3]
                    value = 2 if (own < lo or own > hi) else 0
                out[r, a] |= np.uint32(value << (2 * t))
    return out.view(np.int32)


def match_values(match, T):
    """packed words [R][A] -> values uint8 [T][A][R]"""
    match = np.asarray(match, np.int32)
    match = match.reshape(len(match), -1) if match.ndim != 2 else match
    return np.stack([(match.T >> (2 * t)) & 3 for t in range(T)]).astype(np.uint8)


def accumulate(rows, dataset, thresholds=None, area_ranges=None, max_dets=MAX_DETS):
    """-> precision [T][101][K][A][M], recall [T][K][A][M] (COCOeval.accumulate), -1 where a category has no
    non-ignored ground truth under an area range"""
    thresholds, area_ranges = _limits(thresholds, area_ranges)
    T, A, M = len(thresholds), len(area_ranges), len(max_dets)
    images = dataset["images"]
    K = len(dataset["categories"])
    precision = -np.ones((T, RECALL_POINTS, K, A, M))
    recall = -np.ones((T, K, A, M))
    image = np.asarray(rows["image"], np.int64)
    cls = np.asarray(rows["class"], np.int64)
    score = np.asarray(rows["score"], np.float64)
    values = match_values(rows["match"], T) if len(image) else np.zeros((T, A, 0), np.uint8)
    # rank of a row inside its (image, class) segment: the rows arrive in segment order
    rank = np.zeros(len(image), np.int64)
    for r in range(1, len(image)):
        if image[r] == image[r - 1] and cls[r] == cls[r - 1]:
            rank[r] = rank[r - 1] + 1
        elif (image[r], cls[r]) < (image[r - 1], cls[r - 1]):
            raise ValueError("rows are not in segment order (image, then class) at row %d" % r)
    anns = [o for im in images for o in im["anns"]]                  # every image with a ground truth of k counts
    gt_cls = np.array([o["category"] for o in anns], np.int64)
    gt_area = np.array([o["area"] for o in anns], np.float64)
    gt_crowd = np.array([o["iscrowd"] for o in anns], bool)
    eps = np.spacing(1)
    rec_thrs = np.arange(RECALL_POINTS) / 100.0
    for k in range(K):
        of_k = np.nonzero(cls == k)[0]                      # image ascending, segment order inside: the concatenation
        for a, (lo, hi) in enumerate(area_ranges):
            npig = int(((gt_cls == k) & ~(gt_crowd | (gt_area < lo) | (gt_area > hi))).sum())
            if npig == 0:
                continue
            for m, max_det in enumerate(max_dets):
                sel = of_k[rank[of_k] < max_det]
                sel = sel[np.argsort(-score[sel], kind="mergesort")]
                for t in range(T):
                    v = values[t, a, sel]
                    v = v[v != 2]
                    tp = np.cumsum(v == 1).astype(np.float64)
                    fp = np.cumsum(v == 0).astype(np.float64)
                    rc = tp / npig
                    pr = tp / (fp + tp + eps)
                    recall[t, k, a, m] = rc[-1] if len(rc) else 0
                    for i in range(len(pr) - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    at = np.searchsorted(rc, rec_thrs, side="left")
                    q = np.zeros(RECALL_POINTS)
                    inside = at < len(pr)
                    q[inside] = pr[at[inside]]
                    precision[t, :, k, a, m] = q
    return precision, recall


SUMMARY = (   # (AP or AR, IoU threshold or None for all, area range, maxDet): COCO's order and wording
    (1, None, 0, 100), (1, 0.5, 0, 100), (1, 0.75, 0, 100), (1, None, 1, 100), (1, None, 2, 100), (1, None, 3, 100),
    (0, None, 0, 1), (0, None, 0, 10), (0, None, 0, 100), (0, None, 1, 100), (0, None, 2, 100), (0, None, 3, 100))
AREA_NAMES = ("all", "small", "medium", "large")


def summarize(precision, recall, thresholds=None, max_dets=MAX_DETS):
    """the twelve numbers of COCOeval.summarize in its order (the default thresholds, area ranges and maxDets): each the
    mean over the entries > -1, or -1 where there are none"""
    thresholds = np.asarray(THRESHOLDS if thresholds is None else thresholds, np.float64)
    out = []
    for ap, iou, a, max_det in SUMMARY:
        s = precision if ap else recall
        if iou is not None:
            t = np.nonzero(np.isclose(thresholds, iou))[0]
            if len(t) != 1:
                raise ValueError("summarize needs the IoU threshold %g once among %r" % (iou, thresholds.tolist()))
            s = s[t]
        s = s[..., a, list(max_dets).index(max_det)]
        s = s[s > -1]
        out.append(float(s.mean()) if len(s) else -1.0)
    return out


def summary_lines(stats, thresholds=None):
    """the twelve lines as COCOeval prints them"""
    thresholds = np.asarray(THRESHOLDS if thresholds is None else thresholds, np.float64)
    span = "%0.2f:%0.2f" % (thresholds[0], thresholds[-1])
    lines = []
    for (ap, iou, a, max_det), value in zip(SUMMARY, stats):
        lines.append(" %-18s %s @[ IoU=%-9s | area=%6s | maxDets=%3d ] = %0.3f" % (
            "Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)",
            span if iou is None else "%0.2f" % iou, AREA_NAMES[a], max_det, value))
    return lines


def read_instances(path, image_list=None):
    """an instances_*.json -> {"path", "categories" [K] the original ids ascending, "names" [K], "images": [{"id",
    "file_name", "width", "height", "anns": [{"bbox" [x, y, w, h], "category" index 0..K-1, "area", "iscrowd"}, ...]}, ...]}
    with the images in ascending id (those without annotations kept) and every image's annotations in file order.
    image_list: a Darknet list file (one image path per line); only the images whose file name is the base name of a
    listed path are kept.  A malformed file is a ValueError that names it"""
    try:
        with open(path) as f:
            data = json.load(f)
    except ValueError as e:
        raise ValueError("%s: not a JSON file (%s)" % (path, e))
    if not isinstance(data, dict) or any(not isinstance(data.get(k), list) for k in ("images", "annotations", "categories")):
        raise ValueError("%s: no COCO instances file (it needs the lists images, annotations and categories)" % path)
    try:
        cats = sorted(data["categories"], key=lambda c: c["id"])
        ids = [int(c["id"]) for c in cats]
        if len(set(ids)) != len(ids) or not ids:
            raise ValueError("%s: %d categories, %d distinct ids" % (path, len(ids), len(set(ids))))
        cat_index = {c: k for k, c in enumerate(ids)}
        images = {}
        for im in data["images"]:
            if int(im["id"]) in images:
                raise ValueError("%s: image id %d twice" % (path, im["id"]))
            images[int(im["id"])] = {"id": int(im["id"]), "file_name": str(im["file_name"]), "width": int(im["width"]),
                                     "height": int(im["height"]), "anns": []}
        for n, an in enumerate(data["annotations"]):
            if an["image_id"] not in images:
                raise ValueError("%s: annotation %d names image id %r, which is not in the file" % (path, n, an["image_id"]))
            if an["category_id"] not in cat_index:
                raise ValueError("%s: annotation %d names category id %r, which is not in the file"
                                 % (path, n, an["category_id"]))
            bbox = [float(v) for v in an["bbox"]]
            if len(bbox) != 4:
                raise ValueError("%s: annotation %d has a bbox of %d values" % (path, n, len(bbox)))
            images[an["image_id"]]["anns"].append({"bbox": bbox, "category": cat_index[an["category_id"]],
                                                   "area": float(an["area"]), "iscrowd": int(an.get("iscrowd", 0))})
    except (KeyError, TypeError) as e:
        raise ValueError("%s: malformed record (%s: %s)" % (path, type(e).__name__, e))
    kept = [images[i] for i in sorted(images)]
    if image_list is not None:
        with open(image_list) as f:
            wanted = [os.path.basename(ln.strip()) for ln in f if ln.strip()]
        have = set(im["file_name"] for im in kept)
        missing = [w for w in wanted if w not in have]
        if missing:
            raise ValueError("%s: %s lists %s, which is not an image of the file" % (path, image_list, missing[0]))
        wanted = set(wanted)
        kept = [im for im in kept if im["file_name"] in wanted]
    if not kept:
        raise ValueError("%s: no image" % path)
    return {"path": path, "categories": ids, "names": [str(c.get("name", c["id"])) for c in cats], "images": kept}


def write_results(path, rows, dataset):
    """the JSON array Darknet's `valid` writes for COCO, one object per row in row order, with the image's id, the
    ORIGINAL category id and x, y, w, h of the row form"""
    images, cats = dataset["images"], dataset["categories"]
    with open(path, "w") as f:
        f.write("[\n")
        for r in range(len(rows["score"])):
            x, y, w, h = (float(v) for v in rows["bbox"][r])
            f.write('%s{"image_id":%d, "category_id":%d, "bbox":[%f, %f, %f, %f], "score":%f}' % (
                ",\n" if r else "", images[int(rows["image"][r])]["id"], cats[int(rows["class"][r])], x, y, w, h,
                float(rows["score"][r])))
        f.write("\n]\n")
    return path
