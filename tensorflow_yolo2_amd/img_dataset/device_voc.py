"""Device-resident VOC batches: the decoded images live ONCE, at native resolution, in a uint8 pool in device memory;
every batch -- at any input size -- is produced on the device by two kernels of libyolo2_hip.so
(y2_resize_bilinear_u8_batch, y2_encode_labels: csrc/data.hip).  After start-up the host touches no pixel.

For a fixed size, DeviceVOC(...).get(size) called k times returns bit for bit what
pascal_voc(..., image_size=size, cell_size=size // 32, same flipped / seed / rank / world).get_u8() returns on its k-th
call: both walk pascal_voc.ShardedOrder (one shuffle at start, stride sharding, reshuffle at the wrap), and the kernels
are bit-equal to the host resize and label encoder.  Not in the reference (one image size, cv2 on the host every step);
what it serves is multi-scale training from real images (pascal_train_darknet.py --devkit ... --multi-scale).

With `augment` (an img_dataset.augment.Augment) every sample of every batch gets a parameter row drawn on the host from
the augmentation generator -- crop / pad window, mirror, hue / saturation / exposure -- and the two kernels are
y2_augment_u8_batch and y2_encode_labels_window (csrc/augment.hip), bit-equal to augment.py; the batch order does not
change, and the k-th get(size) still equals the k-th get_u8() of a host batcher built with the same arguments.

The pool, its construction, the list-order batch and the per-call plumbing are DevicePool's (device_pool.py: layout and
entry table there; pool_layout, padded_rows, ALIGN and DEFAULT_MAX_POOL_BYTES are re-exported here).  What is DeviceVOC's
own: with `flipped` the entries of the table are the images followed by their mirrored copies (same offset, flip = 1),
the order of pascal_voc.prepare (build_tables, through _entry_table).  Box table: float64 [entries][max_obj][5] = xmin,
ymin, xmax, ymax, class index in annotation order, and int32 counts [entries].

Evaluation (pascal/pascal_eval_darknet.py) reads the same pool: eval_batch(size, start) resizes the entries start,
start + 1, ... in LIST order with y2_resize_bilinear_u8_batch alone and leaves the shuffled cursor of get() where it is;
`difficult`, uint8 [entries][max_obj] parallel to the box table, goes to the device at its first use (training never
reads it).  Evaluation wants the plain list: a data set with `flipped` or `augment` refuses.  eval_batch(size, start,
letterbox=True) keeps every image's aspect ratio instead (y2_letterbox_u8_batch: csrc/data.hip).  Both are
DevicePool.list_batch; img_dataset/device_images.py is the same pool built from plain image files, without annotations.

With `max_boxes` = T, get(size) returns (images, labels, truth, ntruth): the box list of the anchor model next to the
label grid -- truth float32 [B][T][5] = cx, cy, w, h in pixels of the input and the class index of EVERY object of the
window in annotation order, ntruth int32 [B] (augment.encode_box_list; y2_encode_box_list, csrc/augment.hip).  One more
launch on the same stream and no further upload: the kernel reads the index and parameter tensors of the other two."""
import os
import zlib

import numpy as np

from .device_pool import (ALIGN, DEFAULT_MAX_POOL_BYTES, DevicePool, _ptr, check_size, need_gpu, padded_rows,  # noqa: F401
                          pool_layout, stream_of, upload_async)
from .pascal_voc import CLASSES, ShardedOrder, imread_bgr, read_image_set


def build_tables(entries, offsets, pitches, flipped):
    """entry table int64 [E][5], box table float64 [E][max_obj][5], counts int32 [E]; E = len(entries) * (2 if flipped
    else 1), mirrored copies after the plain ones"""
    n = len(entries)
    copies = 2 if flipped else 1
    max_obj = max(len(e['objs']) for e in entries)
    table = np.zeros((n * copies, 5), np.int64)
    boxes = np.zeros((n * copies, max_obj, 5), np.float64)
    counts = np.zeros(n * copies, np.int32)
    for c in range(copies):
        for k, e in enumerate(entries):
            table[c * n + k] = (offsets[k], e['shape'][0], e['shape'][1], pitches[k], c)
            counts[c * n + k] = len(e['objs'])
            if e['objs']:
                boxes[c * n + k, :len(e['objs'])] = np.asarray(e['objs'], np.float64)
    return table, boxes, counts


def build_difficult(entries, max_obj, flipped):
    """uint8 [E][max_obj]: the `difficult` flag of every object of the box table (0 beyond an entry's count)"""
    n = len(entries)
    out = np.zeros((n * (2 if flipped else 1), max_obj), np.uint8)
    for k, e in enumerate(entries):
        d = e.get('difficult', ())
        out[k, :len(d)] = np.asarray(d, np.uint8)
    if flipped:
        out[n:] = out[:n]
    return out


list_batch = DevicePool.list_batch          # callable as list_batch(ds, who, size, start, letterbox, fill)


class DeviceVOC(DevicePool, ShardedOrder):
    def __init__(self, image_set, batch_size=None, devkit_path=None, flipped=None, seed=0, rank=0, world=1,
                 device="cuda", max_pool_bytes=DEFAULT_MAX_POOL_BYTES, augment=None, max_boxes=None):
        from .. import config as cfg
        self.name = 'voc_2007'
        self.devkit_path = devkit_path or os.path.join('data', 'VOCdevkit')
        self.data_path = os.path.join(self.devkit_path, 'VOC2007')
        assert os.path.exists(self.data_path), 'Path does not exist: {}'.format(self.data_path)
        self.batch_size = cfg.BATCH_SIZE if batch_size is None else batch_size
        self.classes = CLASSES
        self.num_class = len(CLASSES)
        self.flipped = bool(getattr(cfg, "FLIPPED", False)) if flipped is None else bool(flipped)
        self.image_set = image_set
        self.device = device
        self._init_order(seed, rank, world)
        if max_boxes is not None and not 1 <= int(max_boxes) <= 1024:
            raise ValueError("max_boxes %r outside 1..1024" % (max_boxes,))
        self.max_boxes = None if max_boxes is None else int(max_boxes)
        self.augment = augment
        if augment is not None:
            from .augment import generator
            self.aug_rng = generator(seed, rank)            # its own stream: the batch order is that of augment=None
        self.image_index, self.entries = read_image_set(self.data_path, image_set)
        assert self.entries, "no image with objects in %s" % image_set
        self._build_pool(lambda k: imread_bgr(self.entries[k]['imname']), max_pool_bytes)
        self.boxes, self.counts = self._upload(self.boxes), self._upload(self.counts)
        n = len(self.entries)
        gt = [{'imname': self.entries[k % n]['imname'], 'flipped': k >= n, 'entry': k} for k in range(len(self.counts))]
        self.gt_labels = self._start_order(gt)
        self._check_ranks_agree()
        self._buffers = {}
        self._params = {}
        self._lists = {}

    def _entry_table(self):
        """the table with the mirrored copies; the box table and the counts ride along (host arrays until uploaded)"""
        table, self.boxes, self.counts = build_tables(self.entries, self.offsets, self.pitches, self.flipped)
        self.max_obj = self.boxes.shape[1]
        self.difficult_host = build_difficult(self.entries, self.max_obj, self.flipped)
        self._difficult = None
        return table

    def order_digest(self):
        """(number of entries, CRC-32 of the current order): equal on ranks that hold the same list and seed"""
        text = "\n".join("%s %d" % (os.path.basename(g['imname']), g['flipped']) for g in self.gt_labels)
        return len(self.gt_labels), zlib.crc32(text.encode())

    def buffers(self, size):
        """the (images, labels) tensors get(size) writes: kept per size, overwritten by the next get(size)"""
        import torch
        check_size(size)
        if size not in self._buffers:
            S = size // 32
            self._buffers[size] = (
                torch.empty((self.batch_size, size, size, 3), dtype=torch.uint8, device=self.device),
                torch.empty((self.batch_size, S, S, 5 + self.num_class), dtype=torch.float32, device=self.device),
                torch.empty(self.batch_size, dtype=torch.int32, device=self.device))
        return self._buffers[size]

    def _box_list(self, size, index, params, stream):
        """(truth, ntruth) of the batch whose entries `index` holds: one launch behind the label kernel's"""
        import torch
        from .. import _lib
        if size not in self._lists:
            self._lists[size] = (
                torch.empty((self.batch_size, self.max_boxes, 5), dtype=torch.float32, device=self.device),
                torch.empty(self.batch_size, dtype=torch.int32, device=self.device))
        truth, ntruth = self._lists[size]
        _lib.check(_lib.load().y2_encode_box_list(_ptr(self.boxes), _ptr(self.counts), _ptr(self.table), _ptr(index),
                                                  None if params is None else _ptr(params), self.batch_size,
                                                  self.max_obj, size, self.max_boxes, _ptr(truth), _ptr(ntruth), stream))
        return truth, ntruth

    def get(self, size):
        """(images [B, size, size, 3] uint8 BGR, labels [B, S, S, 25] float32), S = size // 32, device tensors written
        on the current stream; asynchronous.  With max_boxes = T also truth [B, T, 5] float32 and ntruth [B] int32.
        With an Augment every sample has one parameter row, drawn in batch order and uploaded as the index is."""
        import torch
        from .. import _lib
        from .augment import ROW
        need_gpu(self.device, "DeviceVOC.get")
        images, labels, index = self.buffers(size)
        aug, params, n = self.augment, None, len(self.entries)
        entries = np.empty(self.batch_size, np.int32)
        rows = np.empty((self.batch_size, ROW), np.float64)
        for k in range(self.batch_size):
            entries[k] = self._next()['entry']
            if aug is not None:
                rows[k] = aug.draw(self.aug_rng, *self.entries[entries[k] % n]['shape'])
        upload_async(index, entries)
        if aug is not None:
            if size not in self._params:
                self._params[size] = torch.empty((self.batch_size, ROW), dtype=torch.float64, device=self.device)
            params = self._params[size]
            upload_async(params, rows)
        lib, stream = _lib.load(), stream_of(images)
        if aug is None:
            image_kernel, label_kernel, window, fill = lib.y2_resize_bilinear_u8_batch, lib.y2_encode_labels, (), ()
        else:                                               # the window kernels: parameter rows after the index, and a fill
            image_kernel, label_kernel = lib.y2_augment_u8_batch, lib.y2_encode_labels_window
            window, fill = (_ptr(params),), (aug.fill,)
        entry = (_ptr(self.table), _ptr(index)) + window
        _lib.check(image_kernel(_ptr(self.pool), *entry, self.batch_size, size, size, *fill, _ptr(images), stream))
        _lib.check(label_kernel(_ptr(self.boxes), _ptr(self.counts), *entry, self.batch_size, self.max_obj, size,
                                size // 32, self.num_class, _ptr(labels), stream))
        if self.max_boxes is not None:
            return (images, labels) + self._box_list(size, index, params, stream)
        return images, labels

    @property
    def difficult(self):
        """uint8 [entries][max_obj] on the device, uploaded at the first use"""
        if self._difficult is None:
            self._difficult = self._upload(self.difficult_host)
        return self._difficult

    def eval_batch(self, size, start, letterbox=False, fill=127, protocol="repo"):
        """(images [B, size, size, 3] uint8 BGR, valid): entries start .. start + B - 1 of the image list IN LIST ORDER,
        resized on the current stream; the last batch repeats its final entry to fill the fixed batch and `valid` is the
        number of slots that are entries of their own.  `eval_index` is the int32 [B] device tensor of the slots' entries
        (the `index` of the detect and match calls).  The cursor of get() is neither read nor moved.  letterbox: the
        aspect ratio is kept and the rest of the square is `fill` (pascal_voc.letterbox_u8; y2_letterbox_u8_batch) --
        the detect calls then take net_size=size; the same buffers, index and refusals.  protocol="darknet": float32
        RGB in [0, 1] through Darknet's letterbox_image instead (DevicePool.list_batch)."""
        if self.flipped or self.augment is not None:
            raise ValueError("evaluation reads the plain image list: build the DeviceVOC with flipped=False, augment=None")
        return self.list_batch("DeviceVOC.eval_batch", size, start, letterbox, fill, protocol)
