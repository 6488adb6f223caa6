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
launch on the same stream and no further upload: the kernel reads the index and parameter tensors of the other two.

The batch code -- get, buffers, _box_list, the tables, eval_batch -- is DeviceBoxes' (device_boxes.py), stated once for
every list of annotated images; DeviceVOC is the constructor that reads a devkit.  build_tables, build_difficult and
list_batch are re-exported here."""
import os

from .device_boxes import DeviceBoxes, build_difficult, build_tables  # noqa: F401
from .device_pool import (ALIGN, DEFAULT_MAX_POOL_BYTES, DevicePool, _ptr, check_size, need_gpu, padded_rows,  # noqa: F401
                          pool_layout, stream_of, upload_async)
from .pascal_voc import CLASSES, ShardedOrder, imread_bgr, read_image_set  # noqa: F401

list_batch = DevicePool.list_batch          # callable as list_batch(ds, who, size, start, letterbox, fill)


class DeviceVOC(DeviceBoxes):
    def __init__(self, image_set, batch_size=None, devkit_path=None, flipped=None, seed=0, rank=0, world=1,
                 device="cuda", max_pool_bytes=DEFAULT_MAX_POOL_BYTES, augment=None, max_boxes=None, draw=False):
        from .. import config as cfg
        self.name = 'voc_2007'
        self.devkit_path = devkit_path or os.path.join('data', 'VOCdevkit')
        self.data_path = os.path.join(self.devkit_path, 'VOC2007')
        assert os.path.exists(self.data_path), 'Path does not exist: {}'.format(self.data_path)
        batch_size = cfg.BATCH_SIZE if batch_size is None else batch_size
        flipped = bool(getattr(cfg, "FLIPPED", False)) if flipped is None else bool(flipped)
        self.image_set = image_set
        self._check_lists(max_boxes, draw)
        self.image_index, entries = read_image_set(self.data_path, image_set)
        assert entries, "no image with objects in %s" % image_set
        self._init_batches(entries, CLASSES, batch_size, flipped, seed, rank, world, device, max_pool_bytes, augment,
                           max_boxes, draw)
