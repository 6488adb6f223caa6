"""A device-resident pool of the images of a COCO instances file, with the tables COCO's evaluation reads
(coco/coco_eval_yolov2.py): the pool, the entry table and the list-order batches are DevicePool's (device_pool.py); the
annotations come from utils/coco_eval.read_instances.  Not in the reference.

Entries are the file's images in ASCENDING IMAGE ID, those without annotations included (their detections are false
positives), restricted to `image_list` -- a Darknet list file such as 5k.txt -- where one is given.  Every image is
decoded ONCE from image_dir / file_name into the uint8 pool at its native resolution; the JSON's height and width must be
the decoded image's.

Tables, on the device with host copies (`*_host`) for utils/coco_eval.accumulate:
    boxes  float64 [entries][max_obj][5] = x, y, w, h, category index 0..K-1, every annotation in file order, in COCO's OWN
           convention (zero-based continuous corner, no + 1 extent) -- not the 1-based inclusive corners of DeviceVOC's table
    area   float64 [entries][max_obj]     the annotation's `area` field (a segmentation's, not w * h)
    crowd  uint8   [entries][max_obj]     iscrowd
    counts int32   [entries]
max_obj is the largest annotation count of an image (at least 1), at most engine.COCO_MAX_OBJECTS.

eval_batch(size, start, letterbox, fill, protocol) goes through DevicePool.list_batch exactly as DeviceVOC.eval_batch
does; `eval_index`, `table`, `num_class`, `classes` (the category names) and `category_ids` (the original ids, ascending:
with the published files the order of coco.names) are named as there.

Training batches are DeviceCOCOTrain's: the same images as the entries of a DeviceBoxes pool (device_boxes.py), with the
annotations converted to that pool's convention by train_entries -- crowd annotations and boxes with w <= 0 or h <= 0
left out, x, y, w, h -> the 1-based corners (x + 1, y + 1, x + w + 1, y + h + 1), the class the category index 0..K-1,
`difficult` all zero.  Images without an object stay (Darknet's negatives).  DeviceCOCO itself stays as it is."""
import os

import numpy as np

from .device_boxes import DeviceBoxes
from .device_pool import DEFAULT_MAX_POOL_BYTES, DevicePool
from .pascal_voc import imread_bgr

MAX_OBJECTS = 256                           # engine.COCO_MAX_OBJECTS (Y2_COCO_MAX_OBJECTS)


def build_tables(images):
    """read_instances' images -> (boxes float64 [E][max_obj][5], area float64 [E][max_obj], crowd uint8 [E][max_obj],
    counts int32 [E])"""
    max_obj = max(1, max(len(im["anns"]) for im in images))
    if max_obj > MAX_OBJECTS:
        worst = max(images, key=lambda im: len(im["anns"]))
        raise ValueError("image %s has %d annotations, the matcher holds at most %d"
                         % (worst["file_name"], max_obj, MAX_OBJECTS))
    boxes = np.zeros((len(images), max_obj, 5), np.float64)
    area = np.zeros((len(images), max_obj), np.float64)
    crowd = np.zeros((len(images), max_obj), np.uint8)
    counts = np.zeros(len(images), np.int32)
    for k, im in enumerate(images):
        counts[k] = len(im["anns"])
        for j, o in enumerate(im["anns"]):
            boxes[k, j, :4] = o["bbox"]
            boxes[k, j, 4] = o["category"]
            area[k, j] = o["area"]
            crowd[k, j] = 1 if o["iscrowd"] else 0
    return boxes, area, crowd, counts


class DeviceCOCO(DevicePool):
    def __init__(self, annotations, image_dir, batch_size, image_list=None, device="cuda",
                 max_pool_bytes=DEFAULT_MAX_POOL_BYTES):
        from ..utils import coco_eval
        if int(batch_size) < 1:
            raise ValueError("batch_size %r must be at least 1" % (batch_size,))
        self.batch_size, self.device = int(batch_size), device
        self.dataset = coco_eval.read_instances(annotations, image_list)
        self.category_ids = list(self.dataset["categories"])
        self.classes = tuple(self.dataset["names"])
        self.num_class = len(self.category_ids)
        images = self.dataset["images"]
        self.image_ids = [im["id"] for im in images]
        self.entries = [{'imname': os.path.join(image_dir, im["file_name"]), 'shape': (im["height"], im["width"]),
                         'id': im["id"]} for im in images]
        self.boxes_host, self.area_host, self.crowd_host, self.counts_host = build_tables(images)
        self.max_obj = self.boxes_host.shape[1]
        self._build_pool(lambda k: imread_bgr(self.entries[k]['imname']), max_pool_bytes)
        self.boxes, self.area = self._upload(self.boxes_host), self._upload(self.area_host)
        self.crowd, self.counts = self._upload(self.crowd_host), self._upload(self.counts_host)

    def eval_batch(self, size, start, letterbox=False, fill=127, protocol="repo"):
        """(images [B, size, size, 3], valid) of the entries start .. start + B - 1 in list order: DeviceVOC.eval_batch"""
        return self.list_batch("DeviceCOCO.eval_batch", size, start, letterbox, fill, protocol)


def train_entries(images, image_dir):
    """read_instances' images -> the entries of a DeviceBoxes pool, in the same order"""
    entries = []
    for im in images:
        objs = [(x + 1, y + 1, x + w + 1, y + h + 1, int(o["category"]))
                for o in im["anns"] if not o["iscrowd"] for (x, y, w, h) in (o["bbox"],) if w > 0 and h > 0]
        entries.append({'imname': os.path.join(image_dir, im["file_name"]), 'shape': (im["height"], im["width"]),
                        'id': im["id"], 'objs': objs, 'difficult': [0] * len(objs)})
    return entries


class DeviceCOCOTrain(DeviceBoxes):
    """the training pool of a COCO instances file: DeviceBoxes over train_entries of coco_eval.read_instances' images
    (ascending image id, restricted to `image_list` where one is given); `classes` are the category names,
    `category_ids` the original ids and `image_ids` the images', as DeviceCOCO names them"""

    def __init__(self, annotations, image_dir, batch_size, image_list=None, flipped=False, seed=0, rank=0, world=1,
                 device="cuda", max_pool_bytes=DEFAULT_MAX_POOL_BYTES, augment=None, max_boxes=None, draw=False):
        from ..utils import coco_eval
        self._check_lists(max_boxes, draw)
        self.dataset = coco_eval.read_instances(annotations, image_list)
        self.category_ids = list(self.dataset["categories"])
        self.image_ids = [im["id"] for im in self.dataset["images"]]
        self.image_index = [os.path.splitext(im["file_name"])[0] for im in self.dataset["images"]]
        self._init_batches(train_entries(self.dataset["images"], image_dir), self.dataset["names"], batch_size, flipped,
                           seed, rank, world, device, max_pool_bytes, augment, max_boxes, draw)
