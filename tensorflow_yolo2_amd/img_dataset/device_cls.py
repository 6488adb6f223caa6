"""Device-resident classifier batches: the decoded images of an image list [(path, label)] live ONCE in the uint8 pool of
DevicePool (device_pool.py: layout, plain entry table, construction, per-call plumbing), the labels in an int32 [entries]
device tensor, and every training batch -- at any size -- is ONE launch of y2_warp_u8_batch (csrc/augment.hip): mirror, rotation, scale, crop, colour and the
labels of the slots.  After start-up the host touches no pixel; per batch it draws the parameter rows
(augment_cls.ClsAugment.draw_batch: one block of uniforms, vector arithmetic) and uploads them with the index.

For equal arguments the k-th get(size) equals the k-th get_u8(size) of the host batcher cls_images (cls_images.py) on both
arrays: both walk pascal_voc.ShardedOrder and the kernel is bit-equal to augment_cls.py.  With augment=None the kernel
forms the plain stretch of every entry itself (params = NULL: augment_cls.identity_row).

eval_batch(size, start) is the plain stretch of the reference's non-augmented image_read in LIST order
(y2_resize_bilinear_u8_batch through DevicePool.list_batch, as DeviceImages.batch(..., letterbox=False)); labels_of(start)
returns the labels of the same slots.  eval_views(size, start, views) is the same walk with V evaluation views per entry
(img_dataset/eval_views.py: stretch, centre crop, ten crops) from one launch of y2_warp_u8_batch."""
import os
import zlib

import numpy as np

from .cls_images import check_items, stored_image
from .device_pool import (DEFAULT_MAX_POOL_BYTES, DevicePool, _ptr, check_size, list_index, need_gpu, stream_of,
                          upload_async)
from .pascal_voc import ShardedOrder, imread_bgr


class DeviceCls(DevicePool, ShardedOrder):
    def __init__(self, items, batch_size, seed=0, rank=0, world=1, device="cuda",
                 max_pool_bytes=DEFAULT_MAX_POOL_BYTES, augment=None, pool_short_side=None):
        self.items = check_items(items, batch_size, pool_short_side)
        self.batch_size, self.device = int(batch_size), device
        self.pool_short_side = pool_short_side
        self._init_order(seed, rank, world)
        self.augment = augment
        if augment is not None:
            from .augment_cls import generator
            self.aug_rng = generator(seed, rank)            # its own stream: the batch order is that of augment=None
        from PIL import Image
        from .cls_images import stored_shape
        shapes = []
        for p, _ in self.items:                             # the header is enough for the layout
            with Image.open(p) as im:
                w, h = im.size
            shapes.append(stored_shape(h, w, pool_short_side))
        self.entries = [{'imname': p, 'shape': s} for (p, _), s in zip(self.items, shapes)]
        self.shapes = np.array(shapes, np.int64)
        # decoded ONCE; no host copy is kept
        self._build_pool(lambda k: stored_image(imread_bgr(self.entries[k]['imname']), pool_short_side), max_pool_bytes)
        self.labels_host = np.array([l for _, l in self.items], np.int32)
        self.labels = self._upload(self.labels_host)
        self.gt_labels = self._start_order([{'imname': p, 'entry': k} for k, (p, _) in enumerate(self.items)])
        self._check_ranks_agree()
        self._buffers = {}
        self._view_buffers = {}

    def order_digest(self):
        """(number of entries, CRC-32 of the current order and its labels): equal on ranks that hold the same list"""
        text = "\n".join("%s %d" % (os.path.basename(g['imname']), self.labels_host[g['entry']]) for g in self.gt_labels)
        return len(self.gt_labels), zlib.crc32(text.encode())

    def buffers(self, size):
        """the (images, labels, index, params) tensors get(size) writes: kept per size, overwritten by the next call"""
        import torch
        from .augment_cls import ROW
        check_size(size)
        if size not in self._buffers:
            self._buffers[size] = (
                torch.empty((self.batch_size, size, size, 3), dtype=torch.uint8, device=self.device),
                torch.empty(self.batch_size, dtype=torch.int32, device=self.device),
                torch.empty(self.batch_size, dtype=torch.int32, device=self.device),
                torch.empty((self.batch_size, ROW), dtype=torch.float64, device=self.device))
        return self._buffers[size]

    def get(self, size):
        """(images [B, size, size, 3] uint8 BGR, labels [B] int32), device tensors written on the current stream by one
        launch; asynchronous: one index upload and, with `augment`, one parameter upload from pinned memory"""
        from .. import _lib
        need_gpu(self.device, "DeviceCls.get")
        images, labels, index, params = self.buffers(size)
        entries = np.array([self._next()['entry'] for _ in range(self.batch_size)], np.int32)
        upload_async(index, entries)
        fill = 127
        if self.augment is not None:
            upload_async(params, self.augment.draw_batch(self.aug_rng, self.shapes[entries], size))
            fill = self.augment.fill
        _lib.check(_lib.load().y2_warp_u8_batch(_ptr(self.pool), _ptr(self.table), _ptr(index),
                                                _ptr(params) if self.augment is not None else None, _ptr(self.labels),
                                                self.batch_size, size, size, fill, _ptr(images), _ptr(labels),
                                                stream_of(images)))
        return images, labels

    def skip_batches(self, k):
        """advance the order and the augmentation stream by k batches, without a launch"""
        for _ in range(int(k) * self.batch_size):
            self._next()
        if self.augment is not None:
            self.augment.skip(self.aug_rng, self.batch_size, k)

    def eval_batch(self, size, start):
        """(images [B, size, size, 3] uint8 BGR, valid): entries start .. start + B - 1 IN LIST ORDER, stretched to size x
        size on the current stream (DeviceVOC.eval_batch's contract: the last batch repeats its final entry, `eval_index`
        holds the slots' entries, the cursor of get() is neither read nor moved)"""
        if self.augment is not None:
            raise ValueError("evaluation reads the plain image list: build the DeviceCls with augment=None")
        return self.list_batch("DeviceCls.eval_batch", size, start, False, 127)

    def eval_views(self, size, start, views="centre", margin=32, fill=127):
        """(images [B * V, size, size, 3] uint8 BGR, valid): slot b * V + v is view v (eval_views.view_rows) of entry
        min(start + b, E - 1) IN LIST ORDER -- the last batch repeats its final entry, `valid` counts the entries that
        are no repeat, the cursor of get() is neither read nor moved.  One launch of y2_warp_u8_batch on the current
        stream with the repeated index and one pinned upload of the B * V parameter rows; the buffers are kept per
        (size, views) and overwritten by the next call; bit-equal to eval_views.view_images."""
        import torch
        from .. import _lib
        from .augment_cls import ROW
        from .eval_views import VIEWS, view_rows
        if self.augment is not None:
            raise ValueError("evaluation reads the plain image list: build the DeviceCls with augment=None")
        need_gpu(self.device, "DeviceCls.eval_views")
        if not (0 <= fill <= 255 and int(fill) == fill):
            raise ValueError("fill %r is not an integer of 0..255" % (fill,))
        n = len(self.entries)
        entries = list_index(start, self.batch_size, n)
        rows = view_rows(self.shapes[entries], size, views, margin)         # (raises for the other arguments)
        V = VIEWS[views]
        slots = self.batch_size * V
        if (size, views) not in self._view_buffers:
            self._view_buffers[(size, views)] = (
                torch.empty((slots, size, size, 3), dtype=torch.uint8, device=self.device),
                torch.empty(slots, dtype=torch.int32, device=self.device),
                torch.empty((slots, ROW), dtype=torch.float64, device=self.device))
        images, index, params = self._view_buffers[(size, views)]
        upload_async(index, np.repeat(entries, V).astype(np.int32))
        upload_async(params, rows.reshape(slots, ROW))
        _lib.check(_lib.load().y2_warp_u8_batch(_ptr(self.pool), _ptr(self.table), _ptr(index), _ptr(params), None, slots,
                                                size, size, int(fill), _ptr(images), None, stream_of(images)))
        return images, min(self.batch_size, n - start)

    def labels_of(self, start):
        """int32 [B] device tensor: the labels of the slots of eval_batch(size, start)"""
        import torch
        idx = list_index(start, self.batch_size, len(self.entries))
        return torch.from_numpy(self.labels_host[idx]).to(self.device)
