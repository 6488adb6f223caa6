"""The host batcher of the classifier path: an image list [(path, label)] (imagenet.read_image_list) walked in
pascal_voc.ShardedOrder, every sample through img_dataset/augment_cls.py on the host.  The specification DeviceCls
(device_cls.py) is tested against: for equal arguments the k-th get_u8(size) here equals its k-th get(size) on both arrays,
for every rank of every world size.

pool_short_side = L0: an image whose short side exceeds L0 is resized ONCE (pascal_voc.resize_bilinear_u8) so that its
short side is L0 and its long side int(long * (L0 / short)), the reference's arithmetic for a scaled side.  What is kept is
the stored image; every crop is cut from it."""
import numpy as np

from .augment_cls import generator, plain_image
from .pascal_voc import ShardedOrder, imread_bgr, resize_bilinear_u8


def stored_shape(h, w, pool_short_side=None):
    """(height, width) an image of h x w is stored at"""
    h, w = int(h), int(w)
    if pool_short_side is None or min(h, w) <= int(pool_short_side):
        return h, w
    L0 = int(pool_short_side)
    if w <= h:
        return max(1, int(h * (float(L0) / w))), L0
    return L0, max(1, int(w * (float(L0) / h)))


def stored_image(img, pool_short_side=None):
    """the decoded image as the pool stores it"""
    h, w = stored_shape(img.shape[0], img.shape[1], pool_short_side)
    return img if (h, w) == img.shape[:2] else resize_bilinear_u8(img, h, w)


def check_items(items, batch_size, pool_short_side):
    items = [(str(p), int(l)) for p, l in items]
    if not items:
        raise ValueError("an empty image list")
    if int(batch_size) < 1:
        raise ValueError("batch_size %r must be at least 1" % (batch_size,))
    if pool_short_side is not None and int(pool_short_side) < 1:
        raise ValueError("pool_short_side %r must be at least 1" % (pool_short_side,))
    return items


class cls_images(ShardedOrder):
    def __init__(self, items, batch_size, seed=0, rank=0, world=1, augment=None, pool_short_side=None):
        self.items = check_items(items, batch_size, pool_short_side)
        self.batch_size = int(batch_size)
        self.pool_short_side = pool_short_side
        self._init_order(seed, rank, world)
        self.augment = augment
        if augment is not None:
            self.aug_rng = generator(seed, rank)            # its own stream: the batch order is that of augment=None
        self.images = [stored_image(imread_bgr(p), pool_short_side) for p, _ in self.items]
        self.shapes = np.array([im.shape[:2] for im in self.images], np.int64)
        self.labels = np.array([l for _, l in self.items], np.int32)
        self.gt_labels = self._start_order([{'imname': p, 'entry': k} for k, (p, _) in enumerate(self.items)])

    def _entries(self):
        return np.array([self._next()['entry'] for _ in range(self.batch_size)], np.int32)

    def get_u8(self, size):
        """(images uint8 [B, size, size, 3] BGR, labels int32 [B])"""
        if size < 32 or size % 32:
            raise ValueError("size %r is not a positive multiple of 32" % (size,))
        entries = self._entries()
        images = np.empty((self.batch_size, size, size, 3), np.uint8)
        if self.augment is None:
            for b, e in enumerate(entries):
                images[b] = plain_image(self.images[e], size)
        else:
            rows = self.augment.draw_batch(self.aug_rng, self.shapes[entries], size)
            for b, e in enumerate(entries):
                images[b] = self.augment.image(self.images[e], rows[b], size)
        return images, self.labels[entries].copy()

    def skip_batches(self, k):
        """advance the order and the augmentation stream by k batches"""
        for _ in range(int(k)):
            self._entries()
        if self.augment is not None:
            self.augment.skip(self.aug_rng, self.batch_size, k)
