"""The region loss on box lists as a specification (utils/region_loss.py yolov2_loss_boxes): tied to the existing oracle
on collision-free lists, its hand-derived gradient against torch autograd, and the collision rules.  No GPU."""
import numpy as np
import pytest

from oracle import ext_ref as X
from tensorflow_yolo2_amd import synthetic
from tensorflow_yolo2_amd.utils import region_loss as RL

ANCHORS = ((1.3221, 1.73145), (3.19275, 4.00944), (5.05587, 8.09892), (9.47112, 4.84053), (11.2364, 10.0071))


def box(cx, cy, w, h, cls):
    return (cx, cy, w, h, float(cls))


def lists(per_image, T=None):
    """[[(cx, cy, w, h, cls), ...], ...] -> (truth [N][T][5] float32, ntruth [N] int32)"""
    T = T or max(1, max(len(r) for r in per_image))
    truth = np.zeros((len(per_image), T, 5), np.float32)
    for i, r in enumerate(per_image):
        if r:
            truth[i, :len(r)] = np.asarray(r, np.float32)
    return truth, np.array([len(r) for r in per_image], np.int32)


def anchor_box(S, size, cell, anchor, scale=1.05, off=(0.5, 0.5), cls=0):
    """a truth at offset `off` inside `cell` = (row, col) whose shape is `scale` times anchor `anchor` (cell units)"""
    aw, ah = ANCHORS[anchor]
    px = size / S
    return box((cell[1] + off[0]) * px, (cell[0] + off[1]) * px, scale * aw * px, scale * ah * px, cls)


@pytest.mark.parametrize("n,S,size", [(3, 5, 160), (4, 13, 416), (2, 19, 608)])
def test_equals_the_grid_oracle_on_collision_free_lists(n, S, size):
    rng = np.random.default_rng(10 * S + n)
    net = rng.standard_normal((n, S, S, 5, 25)) * 0.6
    lab = synthetic.det_labels(n, size, S, 40 + S)
    lab[1] = 0                                                      # an image with no object
    truth, ntruth = RL.grid_to_box_list(lab, 30)
    assert ntruth[1] == 0 and ntruth.sum() == int((lab[..., 0] > 0).sum()) and truth.shape == (n, 30, 5)
    ref_loss, ref_d = X.yolov2_loss(net, lab, ANCHORS, size)
    loss, dnet = RL.yolov2_loss_boxes(net, truth, ntruth, ANCHORS, size)
    assert np.abs(loss - ref_loss).max() < 1e-12 * max(1.0, np.abs(ref_loss).max())
    assert np.abs(dnet - ref_d).max() < 1e-12
    sc = dict(coord_scale=2.0, object_scale=3.0, noobject_scale=0.5, class_scale=1.5, thresh=0.4)
    l2, d2 = RL.yolov2_loss_boxes(net, truth, ntruth, ANCHORS, size, **sc)
    r2, rd2 = X.yolov2_loss(net, lab, ANCHORS, size, **sc)
    assert np.abs(l2 - r2).max() < 1e-12 * max(1.0, np.abs(r2).max()) and np.abs(d2 - rd2).max() < 1e-12
    # the list order does not matter where no slot is contested
    perm = truth.copy()
    for i in range(n):
        perm[i, :ntruth[i]] = truth[i, :ntruth[i]][::-1]
    l3, d3 = RL.yolov2_loss_boxes(net, perm, ntruth, ANCHORS, size)
    assert np.abs(l3 - loss).max() < 1e-12 and np.abs(d3 - dnet).max() < 1e-12


def torch_loss(net, truth, ntruth, anchors, size, sc, area_weight, prior_scale):
    """the same loss re-expressed in torch: decisions (cells, anchors, owners, the noobject mask) and the IoU target are
    constants, everything else is differentiated by autograd"""
    import torch
    t = torch.tensor(net, dtype=torch.float64, requires_grad=True)
    a = np.asarray(anchors, np.float64)
    an = torch.tensor(a)
    n, S, _, B, D = net.shape
    tot = 0
    for i in range(n):
        ti = t[i]
        sx, sy, so = torch.sigmoid(ti[..., 0]), torch.sigmoid(ti[..., 1]), torch.sigmoid(ti[..., 4])
        col = torch.arange(S, dtype=torch.float64)[None, :, None]
        row = torch.arange(S, dtype=torch.float64)[:, None, None]
        px, py = (sx + col).detach(), (sy + row).detach()
        pw, ph = (an[None, None, :, 0] * torch.exp(ti[..., 2])).detach(), (an[None, None, :, 1] * torch.exp(ti[..., 3])).detach()

        def iou(gx, gy, gw, gh):
            iw = torch.clamp(torch.clamp(px + pw / 2, max=gx + gw / 2) - torch.clamp(px - pw / 2, min=gx - gw / 2), min=0)
            ih = torch.clamp(torch.clamp(py + ph / 2, max=gy + gh / 2) - torch.clamp(py - ph / 2, min=gy - gh / 2), min=0)
            inter = iw * ih
            return inter / (pw * ph + gw * gh - inter)
        best = torch.zeros((S, S, B), dtype=torch.float64)
        owned = torch.zeros((S, S, B), dtype=torch.bool)
        for k in range(int(ntruth[i])):
            gx, gy, gw, gh = [float(v) / size * S for v in np.asarray(truth[i, k, :4], np.float64)]
            cls = int(truth[i, k, 4])
            q, r = min(int(gx), S - 1), min(int(gy), S - 1)
            best = torch.maximum(best, iou(gx, gy, gw, gh))
            inter = np.minimum(gw, a[:, 0]) * np.minimum(gh, a[:, 1])
            bs = int(np.argmax(inter / (gw * gh + a[:, 0] * a[:, 1] - inter)))
            if owned[r, q, bs]:
                continue
            owned[r, q, bs] = True
            tt = ti[r, q, bs]
            wgt = sc["coord_scale"] * ((2.0 - (gw / S) * (gh / S)) if area_weight else 1.0)
            tot = tot + wgt * ((sx[r, q, bs] - (gx - q)) ** 2 + (sy[r, q, bs] - (gy - r)) ** 2 +
                               (tt[2] - np.log(gw / a[bs, 0])) ** 2 + (tt[3] - np.log(gh / a[bs, 1])) ** 2)
            tot = tot + sc["object_scale"] * (so[r, q, bs] - iou(gx, gy, gw, gh)[r, q, bs]) ** 2
            tot = tot + sc["class_scale"] * torch.nn.functional.cross_entropy(tt[5:][None], torch.tensor([cls]))
        free = ~owned
        noobj = free & (best <= sc["thresh"])
        tot = tot + sc["noobject_scale"] * (so[noobj] ** 2).sum()
        if prior_scale > 0:
            prior = (sx - 0.5) ** 2 + (sy - 0.5) ** 2 + ti[..., 2] ** 2 + ti[..., 3] ** 2
            tot = tot + prior_scale * prior[free].sum()
    tot = tot / n
    tot.backward()
    return float(tot.detach()), t.grad.numpy()


def collision_lists(S, size):
    """image 0: two truths in cell (2, 1) on different anchors + one elsewhere; image 1: two truths in cell (1, 3) on the
    SAME anchor (the second loses); image 2: empty"""
    return lists([[anchor_box(S, size, (2, 1), 1, off=(0.3, 0.6), cls=4), anchor_box(S, size, (2, 1), 3, off=(0.7, 0.4), cls=9),
                   anchor_box(S, size, (4, 3), 0, cls=1)],
                  [anchor_box(S, size, (1, 3), 2, 1.05, off=(0.35, 0.3), cls=2), anchor_box(S, size, (1, 3), 2, 0.95, off=(0.6, 0.7), cls=17)],
                  []], 4)


@pytest.mark.parametrize("area_weight,prior_scale", [(False, 0.0), (True, 0.0), (False, 0.01), (True, 0.01)])
def test_gradient_matches_torch_autograd(area_weight, prior_scale):
    S, size = 5, 160
    rng = np.random.default_rng(3)
    net = rng.standard_normal((3, S, S, 5, 25)) * 0.5
    truth, ntruth = collision_lists(S, size)
    for sc in (RL.YOLOV2_SCALES, dict(coord_scale=2.0, object_scale=3.0, noobject_scale=0.5, class_scale=1.5, thresh=0.4)):
        loss, dnet = RL.yolov2_loss_boxes(net, truth, ntruth, ANCHORS, size, area_weight=area_weight,
                                          prior_scale=prior_scale, **sc)
        tot, grad = torch_loss(net, truth, ntruth, ANCHORS, size, sc, area_weight, prior_scale)
        assert abs(tot - loss[4]) < 1e-9 * abs(loss[4])
        assert np.abs(dnet - grad).max() < 1e-9
        assert abs(loss[:4].sum() - loss[4]) < 1e-12


def test_collision_rules():
    S, size = 13, 416
    rng = np.random.default_rng(8)
    net = rng.standard_normal((1, S, S, 5, 25)) * 0.5
    cell = (6, 2)
    # two truths of one cell whose shapes are 1.05 x two different VOC anchors: both slots get coord gradients
    a, b = anchor_box(S, size, cell, 1, cls=7), anchor_box(S, size, cell, 3, cls=2)
    truth, ntruth = lists([[a, b]])
    _, d, m = RL.yolov2_loss_boxes(net, truth, ntruth, ANCHORS, size, return_margins=True)
    assert np.abs(d[0, 6, 2, 1, :4]).min() > 0 and np.abs(d[0, 6, 2, 3, :4]).min() > 0
    assert not d[0, 6, 2, (0, 2, 4), :4].any() and not d[0, 6, 2, (0, 2, 4), 5:].any()
    assert m["shape_gap"] > 0.1 and m["cell_edge"] == pytest.approx(0.5)
    # the grid label of the same objects loses the second one
    lab = np.zeros((1, S, S, 25), np.float32)
    lab[0, 6, 2, 0] = 1; lab[0, 6, 2, 1:5] = a[:4]; lab[0, 6, 2, 5 + 7] = 1
    _, dg = X.yolov2_loss(net, lab, ANCHORS, size)
    assert np.abs(dg[0, 6, 2, 1, :4]).min() > 0 and not dg[0, 6, 2, 3, :4].any()
    # two truths with the same best anchor: only the first gets them, and swapping the order swaps which one
    first, second = anchor_box(S, size, cell, 2, 1.05, off=(0.3, 0.3), cls=5), anchor_box(S, size, cell, 2, 0.9, off=(0.7, 0.6), cls=11)
    singles = {}
    for name, one in (("first", first), ("second", second)):
        singles[name] = RL.yolov2_loss_boxes(net, *lists([[one]]), ANCHORS, size)[1][0, 6, 2, 2]
    d12 = RL.yolov2_loss_boxes(net, *lists([[first, second]]), ANCHORS, size)[1][0, 6, 2, 2]
    d21 = RL.yolov2_loss_boxes(net, *lists([[second, first]]), ANCHORS, size)[1][0, 6, 2, 2]
    assert np.array_equal(d12[:4], singles["first"][:4]) and np.array_equal(d21[:4], singles["second"][:4])
    assert np.array_equal(d12[5:], singles["first"][5:]) and np.array_equal(d21[5:], singles["second"][5:])
    assert not np.array_equal(d12[:4], d21[:4])
    # the loser still exempts a pair it overlaps from the noobject term: aim anchor 3 of a NEIGHBOUR cell at the second
    # truth (IoU 1 with it, low with the first), its confidence gradient must be zero although no truth owns it
    net2 = net.copy()
    loser = anchor_box(S, size, cell, 2, 0.9, off=(0.9, 0.5), cls=11)
    gx, gy, gw, gh = [v / size * S for v in loser[:4]]
    t = net2[0, 6, 3, 2]                                          # cell (6, 3): its x offset would have to be negative,
    t[0], t[1] = -30.0, 0.0                                       # so sigmoid -> 0: centre at x = 3.0, y = 6.5
    t[2], t[3] = np.log(gw / ANCHORS[2][0]), np.log(gh / ANCHORS[2][1])
    winner = anchor_box(S, size, cell, 2, 1.2, off=(0.1, 0.5), cls=5)
    with_loser = RL.yolov2_loss_boxes(net2, *lists([[winner, loser]]), ANCHORS, size)
    without = RL.yolov2_loss_boxes(net2, *lists([[winner]]), ANCHORS, size)
    assert with_loser[1][0, 6, 3, 2, 4] == 0 and without[1][0, 6, 3, 2, 4] > 0
    assert with_loser[0][2] < without[0][2]
    assert np.array_equal(with_loser[1][0, 6, 2, 2, :4], without[1][0, 6, 2, 2, :4])     # ... and takes no coord term


def test_margins_and_empty_input():
    S, size = 5, 160
    net = np.random.default_rng(1).standard_normal((2, S, S, 5, 25)) * 0.5
    truth, ntruth = lists([[], []], 3)
    loss, dnet, m = RL.yolov2_loss_boxes(net, truth, ntruth, ANCHORS, size, return_margins=True)
    assert loss[0] == loss[1] == loss[3] == 0 and loss[2] > 0
    assert not dnet[..., :4].any() and not dnet[..., 5:].any() and np.abs(dnet[..., 4]).max() > 0
    assert m["shape_gap"] == np.inf and m["cell_edge"] == np.inf and m["best_thresh"] == pytest.approx(0.6)
    # the prior reaches every slot of an empty image; rows beyond ntruth are not read
    truth[:, :, :] = 7.0
    l2, d2 = RL.yolov2_loss_boxes(net, truth, ntruth, ANCHORS, size, prior_scale=0.01)
    assert l2[0] > 0 and np.abs(d2[..., :4]).min() > 0 and l2[2] == loss[2]
    # a truth on a cell edge and a tie between two anchors show up as zero margins
    tie = lists([[box(64.0, 80.0, 32.0, 32.0, 0)], []])
    m = RL.yolov2_loss_boxes(net, *tie, ((1.0, 2.0), (2.0, 1.0)) + ANCHORS[2:], size, return_margins=True)[2]
    assert m["cell_edge"] == 0 and m["shape_gap"] == 0
