"""What tests/test_coco_eval_host.py and tests/test_gpu_coco_eval.py share: a second, LITERAL restatement of
COCOeval.evaluateImg (ground truths stable-sorted by their ignore flag, one loop with the `break`), to check
utils/coco_eval.match_segment's two-pass form against; seeded random segments; the hand-worked segments with their expected
words written out; and the helpers that turn boxes into detection rows of either row form."""
import numpy as np

from tensorflow_yolo2_amd.utils import coco_eval as CE

ALL_TP, ALL_IG = 0x55555, 0xAAAAA            # value 1 / value 2 under each of the ten default thresholds


def rows_from_xywh(xywh, cls, row_form):
    """boxes [r][4] = x, y, w, h (integers for row_form 0) and classes [r] -> int32 rows [r][6] of that form: the inverse
    of coco_eval.row_xywh.  Word 5 (the candidate) is the row's number"""
    xywh = np.asarray(xywh, np.float64).reshape(-1, 4)
    rows = np.zeros((len(xywh), 6), np.int32)
    if row_form == 0:
        assert np.all(xywh == np.round(xywh)), "integer rows need integer boxes"
        rows[:, 0], rows[:, 1] = xywh[:, 0] + 1, xywh[:, 1] + 1
        rows[:, 2], rows[:, 3] = xywh[:, 0] + xywh[:, 2], xywh[:, 1] + xywh[:, 3]
    else:
        f = np.stack([xywh[:, 0] + 1, xywh[:, 1] + 1, xywh[:, 0] + xywh[:, 2] + 1, xywh[:, 1] + xywh[:, 3] + 1], 1)
        rows[:, :4] = f.astype(np.float32).view(np.int32)
    rows[:, 4] = np.asarray(cls, np.int32)
    rows[:, 5] = np.arange(len(xywh))
    return rows


def evaluate_img_literal(rows, gt, area, crowd, thresholds, area_ranges, row_form):
    """COCOeval.evaluateImg as it is written, per category and area range -> the packed words [r][A]"""
    rows = CE._rows(rows)
    gt = np.asarray(gt, np.float64).reshape(-1, 5)
    area, crowd = np.asarray(area, np.float64).reshape(-1), np.asarray(crowd).reshape(-1).astype(int)
    box = CE.row_xywh(rows, row_form)
    out = np.zeros((len(rows), len(area_ranges)), np.uint32)     # bit 31 is threshold 15's
    for c in sorted(set(rows[:, 4].tolist())):
        dt = [r for r in range(len(rows)) if rows[r, 4] == c]
        g_all = [j for j in range(len(gt)) if gt[j, 4] == c]
        for a, (lo, hi) in enumerate(area_ranges):
            ignore = [1 if (crowd[j] or area[j] < lo or area[j] > hi) else 0 for j in g_all]
            gtind = np.argsort(ignore, kind="mergesort")
            g = [g_all[i] for i in gtind]
            gtIg = np.array([ignore[i] for i in gtind])
            iscrowd = [int(crowd[j]) for j in g]
            ious = np.array([[CE.bbox_iou(box[r], gt[j], bool(crowd[j])) for j in g] for r in dt]).reshape(len(dt), len(g))
            T, G, D = len(thresholds), len(g), len(dt)
            gtm, dtm, dtIg = np.zeros((T, G)), np.zeros((T, D)), np.zeros((T, D))
            for tind, t in enumerate(thresholds):
                for dind in range(D):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind in range(G):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dtIg[tind, dind] = gtIg[m]
                    dtm[tind, dind] = 1
                    gtm[tind, m] = 1
            outside = np.array([box[r, 2] * box[r, 3] < lo or box[r, 2] * box[r, 3] > hi for r in dt]).reshape(1, D)
            dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(outside, T, 0)))
            for tind in range(T):
                for dind, r in enumerate(dt):
                    value = 2 if dtIg[tind, dind] else (1 if dtm[tind, dind] else 0)
                    out[r, a] |= np.uint32(value << (2 * tind))
    return out.view(np.int32)


def random_segment(rng, row_form, max_gt=12, max_rows=20, classes=4):
    """(rows, gt, area, crowd): classes 1..`classes`, 0..max_gt ground truths with crowd regions and small areas among
    them, 0..max_rows rows.  The boxes sit on a coarse grid, so equal IoUs, exact thresholds and repeats occur"""
    m, r = int(rng.integers(0, max_gt + 1)), int(rng.integers(0, max_rows + 1))
    step = 8 if row_form == 0 else 8.5
    gt = np.zeros((m, 5))
    gt[:, 0:2] = rng.integers(0, 8, (m, 2)) * step
    gt[:, 2:4] = rng.integers(1, 7, (m, 2)) * step
    gt[:, 4] = rng.integers(1, classes + 1, m)
    # the area field is a segmentation's: near w * h, sometimes far below it, sometimes past a range's end
    area = gt[:, 2] * gt[:, 3] * rng.choice([1.0, 0.5, 0.25, 4.0, 8.0], m)
    crowd = (rng.random(m) < 0.2).astype(np.uint8)
    xywh, cls = np.zeros((r, 4)), rng.integers(1, classes + 1, r)
    for k in range(r):
        if m and rng.random() < 0.7:                       # a ground truth, shifted by whole grid steps or not at all
            j = int(rng.integers(0, m))
            xywh[k] = gt[j, :4]
            xywh[k, :2] += rng.integers(-1, 2, 2) * step * (rng.random() < 0.5)
            xywh[k, 2:] = np.maximum(xywh[k, 2:] + rng.integers(-1, 2, 2) * step * (rng.random() < 0.3), step)
            xywh[k, :2] = np.maximum(xywh[k, :2], 0)
            if rng.random() < 0.8:
                cls[k] = gt[j, 4]
        else:
            xywh[k, :2] = rng.integers(0, 8, 2) * step
            xywh[k, 2:] = rng.integers(1, 7, 2) * step
    return rows_from_xywh(xywh, cls, row_form), gt, area, crowd


# ---- hand-worked segments: (name, boxes x, y, w, h of the rows, their classes, gt, area, crowd, thresholds, area ranges,
#      expected words).  thresholds / area_ranges None: COCO's ten and four (all, small, medium, large)
HAND = [
    # g0 is a plain 50 x 50 object, g1 a crowd region.  Row 0 is g0 exactly: a true positive where 2500 is inside the area
    # range (all, medium), ignored where g0 is (small, large).  Row 1 is g0 again: g0 is taken and the crowd region is
    # disjoint, so it is a false positive under "all" and "medium", and under "small" and "large" its own area of 2500
    # is outside the range.  Rows 2 and 3 lie inside the crowd region: crowd IoU 1, both absorbed.
    ("crowd absorbs two detections", [[100, 100, 50, 50], [100, 100, 50, 50], [10, 10, 20, 20], [30, 30, 40, 40]], [1, 1, 1, 1],
     [[100, 100, 50, 50, 1], [0, 0, 80, 80, 1]], [2500, 6400], [0, 1], None, None,
     [[ALL_TP, ALL_IG, ALL_TP, ALL_IG], [0, ALL_IG, 0, ALL_IG], [ALL_IG] * 4, [ALL_IG] * 4]),
    # row 0 overlaps g0 and g1 by the same 50 of a union of 150: the LATER one, g1, is matched; row 1 is g1 exactly and
    # finds it taken, and g0 is disjoint from it: a false positive (with g0 matched first it would be a true positive)
    ("equal IoU: the later ground truth", [[5, 0, 10, 10], [10, 0, 10, 10]], [2, 2],
     [[0, 0, 10, 10, 2], [10, 0, 10, 10, 2]], [100, 100], [0, 0], [0.25], [[0, 1e10]], [[1], [0]]),
    # the crowd region g0 overlaps the row fully (crowd IoU 1), the plain g1 by exactly 0.5: g1 is the match at 0.5.  The
    # same box again finds g1 taken and is absorbed by the crowd region
    ("a non-ignored match is not displaced", [[0, 0, 40, 40], [0, 0, 40, 40]], [1, 1],
     [[0, 0, 100, 100, 1], [0, 0, 40, 20, 1]], [10000, 800], [1, 0], [0.5], [[0, 1e10]], [[1], [2]]),
    ("an unmatched 20 x 20 detection", [[0, 0, 20, 20]], [3], np.zeros((0, 5)), [], [], None, None,
     [[0, 0, ALL_IG, ALL_IG]]),
    ("a row of another class", [[0, 0, 50, 50]], [2], [[0, 0, 50, 50, 3]], [2500], [0], None, None,
     [[0, ALL_IG, 0, ALL_IG]]),
    # IoU exactly 0.5: a true positive at the threshold 0.5 and at no other.  Under "medium" and "large" the ground truth
    # (area 2) is ignored: matched at 0.5 (value 2), and elsewhere the row's own area of 4 is outside the range
    ("IoU exactly at the threshold", [[0, 0, 2, 2]], [1], [[0, 0, 2, 1, 1]], [2], [0], None, None,
     [[1, 1, ALL_IG, ALL_IG]]),
]


def hand_case(case, row_form):
    name, xywh, cls, gt, area, crowd, thresholds, area_ranges, expect = case
    return (rows_from_xywh(xywh, cls, row_form), np.asarray(gt, np.float64).reshape(-1, 5), np.asarray(area, np.float64),
            np.asarray(crowd, np.uint8), thresholds, area_ranges, np.asarray(expect, np.int32))


# ---- rows of a whole data set, from the specification
def make_dataset(images):
    """[(image id, [(x, y, w, h, category index, area, iscrowd), ...]), ...] -> read_instances' dict, K = the largest
    category index + 1 (at least 2)"""
    K = max([2] + [int(o[4]) + 1 for _i, anns in images for o in anns])
    return {"path": "made", "categories": [10 * (k + 1) for k in range(K)], "names": ["c%d" % k for k in range(K)],
            "images": [{"id": i, "file_name": "%d.jpg" % i, "width": 640, "height": 480,
                        "anns": [{"bbox": [float(v) for v in o[:4]], "category": int(o[4]), "area": float(o[5]),
                                  "iscrowd": int(o[6])} for o in anns]} for i, anns in sorted(images)]}


def gt_tables(image):
    anns = image["anns"]
    gt = np.array([o["bbox"] + [o["category"]] for o in anns], np.float64).reshape(-1, 5)
    return gt, np.array([o["area"] for o in anns], np.float64), np.array([o["iscrowd"] for o in anns], np.uint8)


def spec_rows(dataset, segments, row_form):
    """segments: [(entry, class, xywh [r][4], scores [r] descending), ...] in segment order -> the rows dict of
    coco_eval.accumulate, every segment matched by coco_eval.match_segment"""
    cols = {k: [] for k in ("image", "class", "score", "match", "bbox")}
    for entry, c, xywh, scores in segments:
        rows = rows_from_xywh(xywh, [c] * len(xywh), row_form)
        gt, area, crowd = gt_tables(dataset["images"][entry])
        cols["match"].append(CE.match_segment(rows, gt, area, crowd, row_form=row_form))
        cols["image"].append(np.full(len(rows), entry))
        cols["class"].append(np.full(len(rows), c))
        cols["score"].append(np.asarray(scores, np.float32))
        cols["bbox"].append(CE.row_xywh(rows, row_form))
    return {k: np.concatenate(v) if v else np.zeros((0, 4)) for k, v in cols.items()}


def rematch(rows, dataset, raw_rows, row_form):
    """the match words of the specification for rows that came back from an evaluation: raw_rows int32 [R][>= 5] are the
    rows' own words, rows["image"] / rows["class"] say which segment each belongs to"""
    out = np.zeros((len(raw_rows), len(CE.AREA_RANGES)), np.int32)
    keys = list(zip(np.asarray(rows["image"]).tolist(), np.asarray(rows["class"]).tolist()))
    for key in sorted(set(keys)):
        sel = np.array([r for r, k in enumerate(keys) if k == key])
        gt, area, crowd = gt_tables(dataset["images"][key[0]])
        out[sel] = CE.match_segment(raw_rows[sel], gt, area, crowd, row_form=row_form)
    return out
