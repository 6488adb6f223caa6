"""The name map of a YOLOv2 snapshot (yolo2_nets/net_utils.save_yolov2_variables / restore_yolov2_variables): numpy only.

One `.npz` holds the three conv-BN-leaky stacks of yolo2_nets/yolov2.py under stable names

    yolov2/<stack>/<layer>/<key>          stack: stem | deep | head;  key: W b gamma beta moving_mean moving_var
    yolov2/anchors  [B][2] float32        yolov2/num_class  int64        yolov2/iteration  int64

and, for a trainer, the optimizer of the composed graph: per stack the two Adam moments of every parameter and its
step count, then the ONE loss scaler the three stacks share

    yolov2/<stack>/<layer>/<key>/Adam     yolov2/<stack>/<layer>/<key>/Adam_1      yolov2/<stack>/adam_step  int64
    yolov2/scaler/ctrl  int32 [8]         yolov2/scaler/scale  float64             yolov2/scaler/clean  int64

(absent in the modes that run without a loss scale).  A trainer on Darknet's solver (utils/solver.py) holds instead, per
stack, the one momentum slot of every parameter and its step count, and once the solver record, every field of it

    yolov2/<stack>/<layer>/<key>/Momentum     yolov2/<stack>/sgd_step  int64
    yolov2/solver/learning_rate, momentum, decay  float32      yolov2/solver/policy  str
    yolov2/solver/burn_in, power, max_batches  int64   yolov2/solver/steps  int64 [n]   yolov2/solver/scales  float32 [n]

A snapshot holds the slots of one optimizer; the Adam names and an Adam snapshot's bytes are what they were.

A model built with another batch-norm epsilon than the contexts' default (YOLOv2Trainer(bn_eps=1e-6), the one a backbone
from a Darknet file needs) adds ONE key, `yolov2/bn_eps` float64; a default model writes no such key, so its snapshots
keep their bytes."""
import numpy as np

STACKS = ("stem", "deep", "head")
PARAM_KEYS = ("W", "b", "gamma", "beta")
STATE_KEYS = ("moving_mean", "moving_var")
PREFIX = "yolov2/"


SOLVER_PREFIX = PREFIX + "solver/"


DEFAULT_BN_EPS = 1e-3            # engine.Network's (tf.layers.batch_normalization's)


def to_blob(stacks, anchors, num_class, iteration, adam=None, scaler=None, sgd=None, solver=None, bn_eps=None):
    """stacks: {stack: [layer dict of the six arrays]}; adam: {stack: {"m": [layer dict of PARAM_KEYS], "v": [...],
    "t": int}} or None; scaler: {"ctrl": int32 [8], "scale": float, "clean": int} or None; sgd: {stack: {"accum": [layer
    dict of PARAM_KEYS], "t": int}} with solver, a utils.solver.Solver, or both None -> flat {name: array}"""
    assert sorted(stacks) == sorted(STACKS), sorted(stacks)
    assert adam is None or sgd is None, "one optimizer per snapshot"
    assert (sgd is None) == (solver is None), "the Momentum slots go with their solver record"
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
        if sgd is not None:
            assert len(sgd[s]["accum"]) == len(stacks[s])
            for l, layer in enumerate(sgd[s]["accum"]):
                for k in PARAM_KEYS:
                    blob["%s%s/%d/%s/Momentum" % (PREFIX, s, l, k)] = np.asarray(layer[k], np.float32)
            blob["%s%s/sgd_step" % (PREFIX, s)] = np.int64(sgd[s]["t"])
    if solver is not None:
        blob.update(solver_to_blob(solver))
    if scaler is not None:
        blob[PREFIX + "scaler/ctrl"] = np.asarray(scaler["ctrl"], np.int32).reshape(8)
        blob[PREFIX + "scaler/scale"] = np.float64(scaler["scale"])
        blob[PREFIX + "scaler/clean"] = np.int64(scaler["clean"])
    if bn_eps is not None and float(bn_eps) != DEFAULT_BN_EPS:
        blob[PREFIX + "bn_eps"] = np.float64(bn_eps)
    return blob


def bn_eps_from_blob(snap):
    """the batch-norm epsilon a snapshot was written with: its `yolov2/bn_eps`, or the default where it has none"""
    return float(snap[PREFIX + "bn_eps"]) if _has(snap, PREFIX + "bn_eps") else DEFAULT_BN_EPS


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


def solver_to_blob(solver):
    """yolov2/solver/*: every field of a utils.solver.Solver, as the C ABI carries it"""
    d = solver.as_dict()
    blob = {SOLVER_PREFIX + k: np.float32(d[k]) for k in ("learning_rate", "momentum", "decay")}
    blob[SOLVER_PREFIX + "policy"] = np.str_(d["policy"])
    for k in ("burn_in", "power", "max_batches"):
        blob[SOLVER_PREFIX + k] = np.int64(d[k])
    blob[SOLVER_PREFIX + "steps"] = np.asarray(d["steps"], np.int64).reshape(-1)
    blob[SOLVER_PREFIX + "scales"] = np.asarray(d["scales"], np.float32).reshape(-1)
    return blob


def sgd_from_blob(snap):
    """(sgd, solver) of a snapshot written with Darknet's solver -- {stack: {"accum": [layer dict of PARAM_KEYS], "t":
    int}} and a utils.solver.Solver -- or (None, None)"""
    from .solver import Solver
    if not _has(snap, SOLVER_PREFIX + "policy"):
        return None, None
    g = lambda k: snap[SOLVER_PREFIX + k]
    solver = Solver(float(g("learning_rate")), float(g("momentum")), float(g("decay")), str(g("policy")), int(g("burn_in")),
                    int(g("power")), tuple(int(v) for v in np.asarray(g("steps")).reshape(-1)),
                    tuple(float(v) for v in np.asarray(g("scales")).reshape(-1)), int(g("max_batches")))
    sgd = {}
    for s in STACKS:
        acc = []
        while _has(snap, "%s%s/%d/W/Momentum" % (PREFIX, s, len(acc))):
            base = "%s%s/%d/" % (PREFIX, s, len(acc))
            acc.append({k: np.asarray(snap[base + k + "/Momentum"], np.float32) for k in PARAM_KEYS})
        if not acc or not _has(snap, "%s%s/sgd_step" % (PREFIX, s)):
            raise ValueError("snapshot with a solver record but no Momentum slots for the %s stack" % s)
        sgd[s] = {"accum": acc, "t": int(snap["%s%s/sgd_step" % (PREFIX, s)])}
    return sgd, solver


def check_optimizer(path, have_adam, have_solver, want_solver):
    """A trainer restores the slots of ITS optimizer only.  have_adam: the snapshot holds Adam slots; have_solver: its
    solver record or None; want_solver: the trainer's record, None for an Adam trainer.  A snapshot without optimizer
    slots (a detector's) passes.  Raises ValueError naming both sides."""
    if want_solver is None and have_solver is not None:
        raise ValueError("snapshot %s holds the Momentum slots of Darknet's solver (%r), the trainer runs Adam" %
                         (path, have_solver))
    if want_solver is not None and have_adam:
        raise ValueError("snapshot %s holds Adam slots, the trainer runs Darknet's solver (%r)" % (path, want_solver))
    if want_solver is not None and have_solver is not None and have_solver != want_solver:
        raise ValueError("snapshot %s: its solver record is %r, the trainer's is %r" % (path, have_solver, want_solver))


def check_matches(what, path, have, want):
    """raise with both values named unless the snapshot's `have` equals the model's `want`"""
    have, want = np.asarray(have), np.asarray(want)
    if have.shape != want.shape or not np.array_equal(have, want):
        raise ValueError("snapshot %s: %s is %s, the model has %s" % (path, what, have.tolist(), want.tolist()))
