"""The name map of a YOLOv2 snapshot (yolo2_nets/net_utils.save_yolov2_variables / restore_yolov2_variables): numpy only.

One `.npz` holds the three conv-BN-leaky stacks of yolo2_nets/yolov2.py under stable names

    yolov2/<stack>/<layer>/<key>          stack: stem | deep | head;  key: W b gamma beta moving_mean moving_var
    yolov2/anchors  [B][2] float32        yolov2/num_class  int64        yolov2/iteration  int64

and, for a trainer, the optimizer of the composed graph: per stack the two Adam moments of every parameter and its
step count, then the ONE loss scaler the three stacks share

    yolov2/<stack>/<layer>/<key>/Adam     yolov2/<stack>/<layer>/<key>/Adam_1      yolov2/<stack>/adam_step  int64
    yolov2/scaler/ctrl  int32 [8]         yolov2/scaler/scale  float64             yolov2/scaler/clean  int64

(absent in the modes that run without a loss scale)."""
import numpy as np

STACKS = ("stem", "deep", "head")
PARAM_KEYS = ("W", "b", "gamma", "beta")
STATE_KEYS = ("moving_mean", "moving_var")
PREFIX = "yolov2/"


def to_blob(stacks, anchors, num_class, iteration, adam=None, scaler=None):
    """stacks: {stack: [layer dict of the six arrays]}; adam: {stack: {"m": [layer dict of PARAM_KEYS], "v": [...],
    "t": int}} or None; scaler: {"ctrl": int32 [8], "scale": float, "clean": int} or None -> flat {name: array}"""
    assert sorted(stacks) == sorted(STACKS), sorted(stacks)
    blob = {PREFIX + "anchors": np.asarray(anchors, np.float32).reshape(-1, 2),
            PREFIX + "num_class": np.int64(num_class), PREFIX + "iteration": np.int64(iteration)}
    for s in STACKS:
        for l, layer in enumerate(stacks[s]):
            for k in PARAM_KEYS + STATE_KEYS:
                blob["%s%s/%d/%s" % (PREFIX, s, l, k)] = np.asarray(layer[k], np.float32)
        if adam is not None:
            for slot, suffix in (("m", "/Adam"), ("v", "/Adam_1")):
                assert len(adam[s][slot]) == len(stacks[s])
                for l, layer in enumerate(adam[s][slot]):
                    for k in PARAM_KEYS:
                        blob["%s%s/%d/%s%s" % (PREFIX, s, l, k, suffix)] = np.asarray(layer[k], np.float32)
            blob["%s%s/adam_step" % (PREFIX, s)] = np.int64(adam[s]["t"])
    if scaler is not None:
        blob[PREFIX + "scaler/ctrl"] = np.asarray(scaler["ctrl"], np.int32).reshape(8)
        blob[PREFIX + "scaler/scale"] = np.float64(scaler["scale"])
        blob[PREFIX + "scaler/clean"] = np.int64(scaler["clean"])
    return blob


def _has(snap, name):
    return name in (snap.files if hasattr(snap, "files") else snap)


def meta_from_blob(snap):
    """(anchors float32 [B][2], num_class, iteration) of a snapshot (a dict or an open .npz)"""
    for k in ("anchors", "num_class", "iteration"):
        if not _has(snap, PREFIX + k):
            raise ValueError("not a YOLOv2 snapshot: %s%s is missing" % (PREFIX, k))
    return (np.asarray(snap[PREFIX + "anchors"], np.float32).reshape(-1, 2), int(snap[PREFIX + "num_class"]),
            int(snap[PREFIX + "iteration"]))


def from_blob(snap):
    """the inverse of to_blob: (stacks, anchors, num_class, iteration, adam or None, scaler or None)"""
    anchors, num_class, iteration = meta_from_blob(snap)
    stacks, adam = {}, {}
    for s in STACKS:
        layers, m, v = [], [], []
        while _has(snap, "%s%s/%d/W" % (PREFIX, s, len(layers))):
            base = "%s%s/%d/" % (PREFIX, s, len(layers))
            layers.append({k: np.asarray(snap[base + k], np.float32) for k in PARAM_KEYS + STATE_KEYS})
            if _has(snap, base + "W/Adam"):
                m.append({k: np.asarray(snap[base + k + "/Adam"], np.float32) for k in PARAM_KEYS})
                v.append({k: np.asarray(snap[base + k + "/Adam_1"], np.float32) for k in PARAM_KEYS})
        if not layers:
            raise ValueError("not a YOLOv2 snapshot: the %s stack is missing" % s)
        stacks[s] = layers
        if len(m) == len(layers) and _has(snap, "%s%s/adam_step" % (PREFIX, s)):
            adam[s] = {"m": m, "v": v, "t": int(snap["%s%s/adam_step" % (PREFIX, s)])}
    scaler = None
    if _has(snap, PREFIX + "scaler/ctrl"):
        scaler = {"ctrl": np.asarray(snap[PREFIX + "scaler/ctrl"], np.int32).reshape(8),
                  "scale": float(snap[PREFIX + "scaler/scale"]), "clean": int(snap[PREFIX + "scaler/clean"])}
    return stacks, anchors, num_class, iteration, (adam if len(adam) == len(STACKS) else None), scaler


def check_matches(what, path, have, want):
    """raise with both values named unless the snapshot's `have` equals the model's `want`"""
    have, want = np.asarray(have), np.asarray(want)
    if have.shape != want.shape or not np.array_equal(have, want):
        raise ValueError("snapshot %s: %s is %s, the model has %s" % (path, what, have.tolist(), want.tolist()))
