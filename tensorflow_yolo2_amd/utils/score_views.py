"""The specification of y2_score_views (csrc/score.hip) in numpy float64: per image the softmax of every view, the mean
over the views, the k best classes, the rank of the label and the counters a validation run accumulates.

  p_v[c] = exp(x_v[c] - max_v) / sum_c exp(x_v[c] - max_v),    p[c] = (1 / V) * sum_v p_v[c]
  order    larger score first, equal scores by the lower class index.  views == 1: the score is the LOGIT (the order of
           tf.nn.top_k and tf.argmax; two logits that round to one probability still rank as the logits do); views > 1:
           the score is p[c] (the kernel orders its own float32 p)
  top_idx, top_val [n, k]   the j-th class in that order and its p; j >= classes: index -1, value 0
  rank [n]                  the number of classes ordered before the label; a label outside 0 .. classes - 1: `classes`
  hits [4]                  accumulated: images, rank == 0, rank < k, labels outside the classes -- slots b < n_valid only
"""
import numpy as np


def score_views_ref(logits, labels=None, views=1, k=5, n_valid=None, hits=None):
    """logits [n * views, classes] (row b * views + v) or [n, views, classes]; labels [n] or None ->
    (top_idx int32 [n, k], top_val float64 [n, k], rank int32 [n] or None, hits int64 [4] or None, prob float64
    [n, classes]).  `hits` (given): the counters so far; a new array is returned."""
    x = np.asarray(logits, np.float64)
    views, k = int(views), int(k)
    classes = x.shape[-1]
    if not 1 <= views <= 16 or not 1 <= k <= 8 or classes < 1 or x.size % (views * classes) or x.size == 0:
        raise ValueError("logits %r with views = %d, k = %d" % (x.shape, views, k))
    x = x.reshape(-1, views, classes)
    n = x.shape[0]
    n_valid = n if n_valid is None else int(n_valid)
    if not 0 <= n_valid <= n:
        raise ValueError("n_valid = %d outside 0..%d" % (n_valid, n))
    e = np.exp(x - x.max(axis=2, keepdims=True))
    prob = (1.0 / views) * (e / e.sum(axis=2, keepdims=True)).sum(axis=1)
    score = x[:, 0] if views == 1 else prob
    order = np.argsort(-score, axis=1, kind="stable")           # equal scores keep the index order
    top_idx = np.full((n, k), -1, np.int32)
    top_val = np.zeros((n, k), np.float64)
    m = min(k, classes)
    top_idx[:, :m] = order[:, :m]
    top_val[:, :m] = np.take_along_axis(prob, order[:, :m], axis=1)
    if labels is None:
        if hits is not None:
            raise ValueError("hits need labels")
        return top_idx, top_val, None, None, prob
    labels = np.asarray(labels, np.int64).reshape(n)
    bad = (labels < 0) | (labels >= classes)
    place = np.argsort(order, axis=1, kind="stable")            # place[b, c]: classes ordered before c
    rank = np.where(bad, classes, place[np.arange(n), np.where(bad, 0, labels)]).astype(np.int32)
    out = np.zeros(4, np.int64) if hits is None else np.array(hits, np.int64).reshape(4).copy()
    r, b = rank[:n_valid], bad[:n_valid]
    out += (n_valid, int((r == 0).sum()), int(((r < k) & ~b).sum()), int(b.sum()))
    return top_idx, top_val, rank, out, prob
