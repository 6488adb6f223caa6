"""The training pool of any list of annotated images: what DeviceVOC (device_voc.py: a VOC devkit), DeviceDarknet (below:
a Darknet image list with its label files) and DeviceCOCOTrain (device_coco.py: a COCO instances file) share.  DeviceBoxes
is built from a plain list of entries {'imname', 'shape': (height, width), 'objs': [(xmin, ymin, xmax, ymax, class)],
'difficult'} plus a tuple of class names, and owns the training batch -- get, buffers, _box_list, the parameter-row
upload and the ShardedOrder walk -- the box table (build_tables, build_difficult) and the list-order evaluation batch;
the pool itself is DevicePool's (device_pool.py).  The batches are described in device_voc.py, whose class they came from
unchanged.

Unlike pascal_voc.read_image_set, a list may hold images WITHOUT objects: they stay (Darknet's negatives; the losses
handle ntruth = 0 and an empty grid), and the box table is at least one row deep.

The draw.  With `max_boxes` = T and `draw`, an image whose window keeps more than T objects does not keep the first T
but Darknet's shuffle-then-cut: every sample gets one uint32 key from a generator of its own (augment.key_generator),
and the box-list launch is y2_encode_box_list_draw, which keeps the T objects that rank first under the key, in
annotation order (augment.encode_box_list_draw).  One key per sample is drawn whatever the sample holds, so a resumed run
can move the stream by counting samples; the batch order and the augmentation rows do not move."""
import os
import zlib

import numpy as np

from .device_pool import DEFAULT_MAX_POOL_BYTES, DevicePool, _ptr, check_size, need_gpu, stream_of, upload_async
from . import pascal_voc
from .pascal_voc import ShardedOrder


def build_tables(entries, offsets, pitches, flipped):
    """entry table int64 [E][5], box table float64 [E][max_obj][5], counts int32 [E]; E = len(entries) * (2 if flipped
    else 1), mirrored copies after the plain ones; max_obj is at least 1"""
    n = len(entries)
    copies = 2 if flipped else 1
    max_obj = max(1, max(len(e['objs']) for e in entries))
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


class DeviceBoxes(DevicePool, ShardedOrder):
    def __init__(self, entries, classes, batch_size, flipped=False, seed=0, rank=0, world=1, device="cuda",
                 max_pool_bytes=DEFAULT_MAX_POOL_BYTES, augment=None, max_boxes=None, draw=False):
        self._check_lists(max_boxes, draw)
        self._init_batches(entries, classes, batch_size, flipped, seed, rank, world, device, max_pool_bytes, augment,
                           max_boxes, draw)

    @staticmethod
    def _check_lists(max_boxes, draw):
        if max_boxes is not None and not 1 <= int(max_boxes) <= 1024:
            raise ValueError("max_boxes %r outside 1..1024" % (max_boxes,))
        if draw and max_boxes is None:
            raise ValueError("draw=True chooses among the objects of a box list: it needs max_boxes")

    def _init_batches(self, entries, classes, batch_size, flipped, seed, rank, world, device, max_pool_bytes, augment,
                      max_boxes, draw=False):
        """everything behind the entry list: order, generators, pool, tables, the first shuffle"""
        if int(batch_size) < 1:
            raise ValueError("batch_size %r must be at least 1" % (batch_size,))
        self.entries = list(entries)
        assert self.entries, "no image"
        self.classes, self.num_class = tuple(classes), len(classes)
        self.batch_size, self.flipped, self.device = batch_size, bool(flipped), device
        self._init_order(seed, rank, world)
        self.max_boxes = None if max_boxes is None else int(max_boxes)
        self.draw = bool(draw)
        self.augment = augment
        if augment is not None:
            from .augment import generator
            self.aug_rng = generator(seed, rank)            # its own stream: the batch order is that of augment=None
        if self.draw:
            from .augment import key_generator
            self.key_rng = key_generator(seed, rank)        # and the keys' own: the rows above do not move either
        self._build_pool(lambda k: pascal_voc.imread_bgr(self.entries[k]['imname']), max_pool_bytes)
        self.boxes, self.counts = self._upload(self.boxes), self._upload(self.counts)
        n = len(self.entries)
        gt = [{'imname': self.entries[k % n]['imname'], 'flipped': k >= n, 'entry': k} for k in range(len(self.counts))]
        self.gt_labels = self._start_order(gt)
        self._check_ranks_agree()
        self._buffers = {}
        self._params = {}
        self._lists = {}
        self._keys = {}
        self.last_keys = None

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

    def _box_list(self, size, index, params, stream, keys=None):
        """(truth, ntruth) of the batch whose entries `index` holds: one launch behind the label kernel's.  keys: the
        batch's uint32 keys on the device (the draw), or None"""
        import torch
        from .. import _lib
        if size not in self._lists:
            self._lists[size] = (
                torch.empty((self.batch_size, self.max_boxes, 5), dtype=torch.float32, device=self.device),
                torch.empty(self.batch_size, dtype=torch.int32, device=self.device))
        truth, ntruth = self._lists[size]
        window = None if params is None else _ptr(params)
        if keys is None:
            _lib.check(_lib.load().y2_encode_box_list(_ptr(self.boxes), _ptr(self.counts), _ptr(self.table), _ptr(index),
                                                      window, self.batch_size, self.max_obj, size, self.max_boxes,
                                                      _ptr(truth), _ptr(ntruth), stream))
        else:
            _lib.check(_lib.load().y2_encode_box_list_draw(_ptr(self.boxes), _ptr(self.counts), _ptr(self.table),
                                                           _ptr(index), window, _ptr(keys), self.batch_size, self.max_obj,
                                                           size, self.max_boxes, _ptr(truth), _ptr(ntruth), stream))
        return truth, ntruth

    def next_sample(self):
        """(entry, parameter row or None, key or None) of the next sample: the order's next entry and, in this order, the
        draws of its augmentation row and of its key.  get() calls it once per slot; a resumed run calls it to move a
        fresh pool to where the saved run stood"""
        from .augment import draw_key
        entry = self._next()['entry']
        row = key = None
        if self.augment is not None:
            row = self.augment.draw(self.aug_rng, *self.entries[entry % len(self.entries)]['shape'])
        if self.draw:
            key = draw_key(self.key_rng)
        return entry, row, key

    def get(self, size):
        """(images [B, size, size, 3] uint8 BGR, labels [B, S, S, 5 + C] float32), S = size // 32, device tensors written
        on the current stream; asynchronous.  With max_boxes = T also truth [B, T, 5] float32 and ntruth [B] int32.
        With an Augment every sample has one parameter row, drawn in batch order and uploaded as the index is; with the
        draw one uint32 key likewise (`last_keys`: the host copy of the last batch's)."""
        import torch
        from .. import _lib
        from .augment import ROW
        need_gpu(self.device, "%s.get" % type(self).__name__)
        images, labels, index = self.buffers(size)
        aug, params, keys = self.augment, None, None
        entries = np.empty(self.batch_size, np.int32)
        rows = np.empty((self.batch_size, ROW), np.float64)
        host_keys = np.empty(self.batch_size, np.uint32) if self.draw else None
        for k in range(self.batch_size):
            entries[k], row, key = self.next_sample()
            if aug is not None:
                rows[k] = row
            if self.draw:
                host_keys[k] = key
        upload_async(index, entries)
        if aug is not None:
            if size not in self._params:
                self._params[size] = torch.empty((self.batch_size, ROW), dtype=torch.float64, device=self.device)
            params = self._params[size]
            upload_async(params, rows)
        if self.draw:
            if size not in self._keys:          # uint32 bits in an int32 tensor
                self._keys[size] = torch.empty(self.batch_size, dtype=torch.int32, device=self.device)
            keys = self._keys[size]
            upload_async(keys, host_keys.view(np.int32))
            self.last_keys = host_keys
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
            return (images, labels) + self._box_list(size, index, params, stream, keys)
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
        who = type(self).__name__
        if self.flipped or self.augment is not None:
            raise ValueError("evaluation reads the plain image list: build the %s with flipped=False, augment=None" % who)
        return self.list_batch("%s.eval_batch" % who, size, start, letterbox, fill, protocol)


class DeviceDarknet(DeviceBoxes):
    """the pool of a Darknet image list: one image path per line of `list_path`, every image's objects in the label file
    Darknet's rule names (utils/darknet_data.py: read_list, label_path, read_labels, to_pixel_boxes).  classes: the
    class count of the .data file; names: the class names (default "0", "1", ...), whose count must be `classes`.
    `image_index`: the images' file names without extension, the ids of a results file.  labels=False: no label file is
    read and every entry is without objects (a list that is only detected on)"""

    def __init__(self, list_path, classes, names=None, batch_size=1, flipped=False, seed=0, rank=0, world=1,
                 device="cuda", max_pool_bytes=DEFAULT_MAX_POOL_BYTES, augment=None, max_boxes=None, draw=False,
                 labels=True):
        from ..utils import darknet_data
        self._check_lists(max_boxes, draw)
        classes = int(classes)
        names = tuple(str(c) for c in range(classes)) if names is None else tuple(names)
        if len(names) != classes:
            raise ValueError("%d names for classes=%d" % (len(names), classes))
        self.list_path = list_path
        entries = darknet_data.image_entries(list_path, classes, labels)
        if not entries:
            raise ValueError("%s: no image" % list_path)
        self.image_index = [os.path.splitext(os.path.basename(e['imname']))[0] for e in entries]
        self._init_batches(entries, names, batch_size, flipped, seed, rank, world, device, max_pool_bytes, augment,
                           max_boxes, draw)
