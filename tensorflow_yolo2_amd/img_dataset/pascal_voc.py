"""Host-side VOC label encoder and image preprocessing -- the data formats on the
input side of the hot path (src/img_dataset/pascal_voc.py:60-67,125-165).  Pure
numpy host code (the reference's is numpy/cv2 too); file IO over a real VOCdevkit
is out of scope (no dataset here), but everything that touches the arithmetic is
kept: the [S,S,25] grid, first-object-wins, no `difficult` filtering."""
import xml.etree.ElementTree as ET

import numpy as np

CLASSES = ('aeroplane', 'bicycle', 'bird', 'boat',
           'bottle', 'bus', 'car', 'cat', 'chair',
           'cow', 'diningtable', 'dog', 'horse',
           'motorbike', 'person', 'pottedplant',
           'sheep', 'sofa', 'train', 'tvmonitor')       # pascal_voc.py:23-27


def encode_boxes(objs, im_h, im_w, image_size, cell_size, num_class=20):
    """load_pascal_annotation's arithmetic (pascal_voc.py:133-165).
    objs: (xmin, ymin, xmax, ymax, class_index) in 1-based pixels of the original image."""
    h_ratio = 1.0 * image_size / im_h
    w_ratio = 1.0 * image_size / im_w
    label = np.zeros((cell_size, cell_size, 5 + num_class))
    for (xmin, ymin, xmax, ymax, cls_ind) in objs:
        x1 = max(min((float(xmin) - 1) * w_ratio, image_size - 1), 0)
        y1 = max(min((float(ymin) - 1) * h_ratio, image_size - 1), 0)
        x2 = max(min((float(xmax) - 1) * w_ratio, image_size - 1), 0)
        y2 = max(min((float(ymax) - 1) * h_ratio, image_size - 1), 0)
        boxes = [(x2 + x1) / 2.0, (y2 + y1) / 2.0, x2 - x1, y2 - y1]
        x_ind = int(boxes[0] * cell_size / image_size)
        y_ind = int(boxes[1] * cell_size / image_size)
        if label[y_ind, x_ind, 0] == 1:
            continue
        label[y_ind, x_ind, 0] = 1
        label[y_ind, x_ind, 1:5] = boxes
        label[y_ind, x_ind, 5 + cls_ind] = 1
    return label


def parse_annotation(xml_path_or_text, im_shape=None):
    """(object list [(xmin, ymin, xmax, ymax, class_index)] in annotation order, (height, width)).  The reference opens
    the JPEG only for its shape (pascal_voc.py:131-134); the XML's <size> carries the same numbers."""
    text = xml_path_or_text
    if "<annotation" not in text:
        with open(xml_path_or_text) as f:
            text = f.read()
    root = ET.fromstring(text)
    if im_shape is None:
        size = root.find('size')
        im_shape = (int(size.find('height').text), int(size.find('width').text))
    objs = []
    for obj in root.findall('object'):
        bb = obj.find('bndbox')
        cls_ind = CLASSES.index(obj.find('name').text.lower().strip())
        objs.append((float(bb.find('xmin').text), float(bb.find('ymin').text),
                     float(bb.find('xmax').text), float(bb.find('ymax').text), cls_ind))
    return objs, (int(im_shape[0]), int(im_shape[1]))


def parse_difficult(xml_path_or_text):
    """the <difficult> flag (0 / 1) of every object in annotation order, parallel to parse_annotation's list; an object
    without the element counts as 0.  The reference never reads it (no evaluation); the devkit's protocol needs it."""
    text = xml_path_or_text
    if "<annotation" not in text:
        with open(xml_path_or_text) as f:
            text = f.read()
    out = []
    for obj in ET.fromstring(text).findall('object'):
        d = obj.find('difficult')
        out.append(1 if d is not None and d.text is not None and int(d.text.strip() or 0) else 0)
    return out


def load_pascal_annotation(xml_path_or_text, image_size, cell_size, im_shape=None):
    """(label [S,S,25], number of objects)"""
    objs, im_shape = parse_annotation(xml_path_or_text, im_shape)
    return encode_boxes(objs, im_shape[0], im_shape[1], image_size, cell_size), len(objs)


def read_image_set(data_path, image_set):
    """The image list of pascal_voc.load_labels (:87-124) without the encoding: (image_index, entries), one entry
    {'imname', 'objs', 'shape': (height, width), 'difficult'} per image of ImageSets/Main/<image_set>.txt that has
    objects (images without any are dropped, :116-118), in list order.  'difficult' is a list of 0 / 1 parallel to
    'objs' (parse_difficult): training ignores it as the reference does, the evaluation needs it."""
    import os
    txtname = os.path.join(data_path, 'ImageSets', 'Main', image_set + '.txt')
    assert os.path.exists(txtname), 'Path does not exist: {}'.format(txtname)
    with open(txtname) as f:
        image_index = [x.strip() for x in f.readlines() if x.strip()]
    entries = []
    for index in image_index:
        imname = os.path.join(data_path, 'JPEGImages', index + '.jpg')
        xml = os.path.join(data_path, 'Annotations', index + '.xml')
        # the reference reads the JPEG for its shape (:131-134); the header is enough
        from PIL import Image
        with Image.open(imname) as im:
            w, h = im.size
        objs, shape = parse_annotation(xml, im_shape=(h, w))
        if len(objs) == 0:
            continue
        difficult = parse_difficult(xml)
        assert len(difficult) == len(objs), xml
        entries.append({'imname': imname, 'objs': objs, 'shape': shape, 'difficult': difficult})
    return image_index, entries


class ShardedOrder(object):
    """The order in which a batcher walks `self.gt_labels` (pascal_voc.py:42-58,86 plus the round-6 stride sharding):
    one shuffle at start, rank r reads positions r, r + world, ... (len // world of them per epoch), one reshuffle at
    every wrap of the cursor.  The list entries are opaque here; a shuffle consumes the generator by the list's LENGTH
    alone, so two batchers over lists of equal length with equal seeds walk the same permutation."""

    def _init_order(self, seed, rank, world):
        assert world >= 1 and 0 <= rank < world, (rank, world)
        self.rank, self.world = int(rank), int(world)
        self.rng = np.random.default_rng(seed)
        self.cursor = 0

    def _start_order(self, gt_labels):
        self.rng.shuffle(gt_labels)
        self.per_rank = len(gt_labels) // self.world      # positions of one epoch on every rank
        assert self.per_rank >= 1, "fewer images (%d) than ranks (%d)" % (len(gt_labels), self.world)
        return gt_labels

    def _next(self):
        g = self.gt_labels[self.cursor * self.world + self.rank]
        self.cursor += 1
        if self.cursor >= self.per_rank:
            self.rng.shuffle(self.gt_labels)
            self.cursor = 0
        return g


def resize_bilinear_u8(img, out_h, out_w):
    """cv2.resize(img, (w, h)) INTER_LINEAR on uint8 (pascal_voc.py:62): half-pixel
    centres, no antialias, 11-bit fixed-point coefficients (OpenCV's documented scheme)."""
    img = np.asarray(img)
    in_h, in_w = img.shape[:2]

    def coeffs(n_in, n_out):
        f = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5
        i0 = np.floor(f).astype(np.int64)
        frac = np.where(i0 < 0, 0.0, f - i0)
        w1 = np.rint(frac * 2048).astype(np.int64)
        return np.clip(i0, 0, n_in - 1), np.clip(i0 + 1, 0, n_in - 1), 2048 - w1, w1

    y0, y1, wy0, wy1 = coeffs(in_h, out_h)
    x0, x1, wx0, wx1 = coeffs(in_w, out_w)
    a = img.astype(np.int64)
    r0, r1 = a[y0], a[y1]
    top = r0[:, x0] * wx0[None, :, None] + r0[:, x1] * wx1[None, :, None]
    bot = r1[:, x0] * wx0[None, :, None] + r1[:, x1] * wx1[None, :, None]
    return ((top * wy0[:, None, None] + bot * wy1[:, None, None] + (1 << 21)) >> 22).astype(np.uint8)


def letterbox_geometry(im_h, im_w, size):
    """(new_w, new_h, ox, oy) of an im_w x im_h image letterboxed into a size x size input, in integers only, as
    Darknet's letterbox_image: the longer side becomes `size`, the other keeps the aspect ratio (floor division, at
    least 1); ox / oy are the left / top bars and the right / bottom bar gets the odd pixel.  The restatement of
    csrc/letterbox.h (y2_letterbox_geometry)."""
    im_h, im_w, size = int(im_h), int(im_w), int(size)
    if im_h < 1 or im_w < 1 or size < 1:
        raise ValueError("letterbox_geometry: image %d x %d, size = %d: every value must be at least 1" % (im_w, im_h, size))
    if size * im_h <= size * im_w:
        new_w, new_h = size, max(1, (im_h * size) // im_w)
    else:
        new_h, new_w = size, max(1, (im_w * size) // im_h)
    return new_w, new_h, (size - new_w) // 2, (size - new_h) // 2


def letterbox_u8(img, size, fill=127):
    """[H, W, 3] uint8 -> the [size, size, 3] letterboxed input: a canvas of `fill` whose rows oy .. oy + new_h - 1 and
    columns ox .. ox + new_w - 1 (letterbox_geometry) hold resize_bilinear_u8(img, new_h, new_w).  A letterbox in
    DESTINATION space: the picture's edge is not blended with the fill.  `fill` defaults to 127 as Augment's does;
    Darknet's 0.5 lies between 127 and 128.  The specification of y2_letterbox_u8_batch (csrc/data.hip)."""
    img = np.asarray(img)
    if not 0 <= int(fill) <= 255:
        raise ValueError("letterbox_u8: fill = %r outside 0..255" % (fill,))
    new_w, new_h, ox, oy = letterbox_geometry(img.shape[0], img.shape[1], size)
    out = np.full((int(size), int(size), 3), int(fill), np.uint8)
    out[oy:oy + new_h, ox:ox + new_w] = resize_bilinear_u8(img, new_h, new_w)
    return out


def letterbox_darknet(img, size):
    """[H, W, 3] uint8 BGR -> the [size, size, 3] float32 RGB input in [0, 1] that Darknet's `letterbox_image` makes: a
    canvas of 0.5 whose rectangle letterbox_geometry names holds Darknet's `resize_image` of the picture.  All float32,
    no fused multiply-add:
      src(x, y, k) = float32(byte of channel 2 - k) / 255
      horizontal, per source row: w_scale = float(W - 1) / float(new_w - 1); column c: sx = float(c) * w_scale,
        ix = int(sx), dx = sx - float(ix), part = (1 - dx) * src(ix) + dx * src(ix + 1); the LAST column (and every
        column of a source one pixel wide) is src(W - 1), copied
      vertical: h_scale = float(H - 1) / float(new_h - 1); row r: sy = float(r) * h_scale, iy = int(sy),
        dy = sy - float(iy), v = (1 - dy) * part(iy), and v = v + dy * part(iy + 1) UNLESS r is the last row (or H is 1).
    The quirk stays: the last row never receives the second term, so where float(new_h - 1) * h_scale rounds to just
    below H - 1 it is (1 - dy) * part(iy) with dy ~ 1, nearly black ((H, new_h) = (8, 24) is the smallest pair).
    Published weights were scored on such inputs.  Where Darknet is undefined: an output extent of 1 takes the scale 0
    (it would divide by zero), and ix, iy and their + 1 neighbours are clamped to the last column / row (unreachable
    with a non-zero weight).  The specification of y2_letterbox_darknet_batch (csrc/darknet_io.hip), bit for bit."""
    img = np.asarray(img)
    assert img.ndim == 3 and img.shape[2] == 3 and img.dtype == np.uint8, (img.shape, img.dtype)
    f = np.float32
    H, W = img.shape[:2]
    new_w, new_h, ox, oy = letterbox_geometry(H, W, size)
    src = img[:, :, ::-1].astype(f) / f(255.0)                            # [H][W][3] RGB
    w_scale = f(W - 1) / f(new_w - 1) if new_w > 1 else f(0.0)
    h_scale = f(H - 1) / f(new_h - 1) if new_h > 1 else f(0.0)
    sx = np.arange(new_w).astype(f) * w_scale
    ix = sx.astype(np.int64)
    dx = (sx - ix.astype(f))[None, :, None]
    ix0, ix1 = np.minimum(ix, W - 1), np.minimum(ix + 1, W - 1)
    part = (f(1.0) - dx) * src[:, ix0] + dx * src[:, ix1]                 # [H][new_w][3]
    part[:, new_w - 1] = src[:, W - 1]
    if W == 1:
        part[:] = src[:, :1]
    sy = np.arange(new_h).astype(f) * h_scale
    iy = sy.astype(np.int64)
    dy = (sy - iy.astype(f))[:, None, None]
    iy0, iy1 = np.minimum(iy, H - 1), np.minimum(iy + 1, H - 1)
    pic = (f(1.0) - dy) * part[iy0]
    if H != 1:
        pic[:new_h - 1] = pic[:new_h - 1] + dy[:new_h - 1] * part[iy1[:new_h - 1]]
    assert pic.dtype == np.float32
    out = np.full((int(size), int(size), 3), 0.5, np.float32)
    out[oy:oy + new_h, ox:ox + new_w] = pic
    return out


def image_read(image_bgr_u8, image_size, flipped=False):
    """pascal_voc.image_read (:60-67) on an already decoded BGR uint8 array."""
    image = resize_bilinear_u8(image_bgr_u8, image_size, image_size).astype(np.float32)
    image = (image / 255.0) * 2.0 - 1.0
    return image[:, ::-1, :] if flipped else image


def imread_bgr(path):
    """cv2.imread(imname) (pascal_voc.py:61): uint8 [H,W,3] in BGR order.  Decoder: PIL (no OpenCV in this image);
    libjpeg builds may differ by one level on some pixels, which is why the C1 fixture pins the DECODED input."""
    from PIL import Image
    with Image.open(path) as im:
        rgb = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return np.ascontiguousarray(rgb[:, :, ::-1])


def flip_label(label, image_size):
    """the flipped copy of a label grid (pascal_voc.prepare, :74-84): columns mirrored, x -> image_size - 1 - x"""
    out = label[:, ::-1, :].copy()
    resp = out[:, :, 0] == 1
    out[:, :, 1] = np.where(resp, image_size - 1 - out[:, :, 1], out[:, :, 1])
    return out


class pascal_voc(ShardedOrder):
    """The batcher of src/img_dataset/pascal_voc.py:13-86 (`imdb.get()` feeds one sess.run per step,
    pascal_train_darknet.py:96-102): VOC2007 devkit layout (ImageSets/Main/<image_set>.txt, JPEGImages/<i>.jpg,
    Annotations/<i>.xml), images without objects dropped (:116-118), optional flip duplication (:72-85), one
    shuffle at start and one at every wrap of the cursor (:55-57,86).

    get() returns the reference's (images [B,size,size,3] float32 in [-1,1], labels [B,S,S,25]); get_u8() returns
    the same batch with the images still uint8 BGR (resized, before / 255 * 2 - 1) for y2_forward_u8, which
    applies that conversion on the device.  Decoded + resized images are kept in host memory after their first
    use (cache_images; 520 KB per 416x416 image) -- the reference re-decodes every time.

    Data parallelism (round 6; not in the reference): `rank` / `world` shard every epoch by stride.
    All ranks hold the SAME shuffled list (same seed, same number of shuffles: the generator streams stay in lockstep);
    rank r reads positions r, r + world, r + 2 world, ... of it, len // world positions per epoch on every rank (the
    < world entries at the tail of an epoch's order are skipped that epoch -- another order the next one), then all
    reshuffle together.  world = 1 is the reference's cursor, entry for entry."""

    def __init__(self, image_set, batch_size=None, rebuild=False, devkit_path=None, image_size=None, cell_size=None,
                 flipped=None, seed=0, cache_images=True, rank=0, world=1, augment=None, max_boxes=None):
        import os
        from .. import config as cfg
        self.name = 'voc_2007'
        self.devkit_path = devkit_path or os.path.join('data', 'VOCdevkit')
        self.data_path = os.path.join(self.devkit_path, 'VOC2007')
        self.batch_size = cfg.BATCH_SIZE if batch_size is None else batch_size
        self.image_size = cfg.IMAGE_SIZE if image_size is None else image_size
        self.cell_size = (self.image_size // 32) if cell_size is None else cell_size
        self.classes = CLASSES
        self.num_class = len(CLASSES)
        self.class_to_ind = dict(zip(self.classes, range(self.num_class)))
        self.flipped = bool(getattr(cfg, "FLIPPED", False)) if flipped is None else bool(flipped)
        self.image_set = image_set
        self._init_order(seed, rank, world)
        self.cache_images = cache_images
        self._cache = {}
        # the anchor model's box list next to the grid (img_dataset/augment.encode_box_list; not in the reference): with
        # max_boxes = T, get() and get_u8() return (images, labels, truth [B,T,5] float32, ntruth [B] int32)
        if max_boxes is not None and not 1 <= int(max_boxes) <= 1024:
            raise ValueError("max_boxes %r outside 1..1024" % (max_boxes,))
        self.max_boxes = None if max_boxes is None else int(max_boxes)
        self.augment = augment
        if augment is not None:
            from .augment import generator
            self.aug_rng = generator(seed, rank)            # its own stream: the batch order is that of augment=None
            self._decoded = {}
        assert os.path.exists(self.data_path), 'Path does not exist: {}'.format(self.data_path)
        self.gt_labels = self.prepare()

    # ---- pascal_voc.py:69-124
    def load_labels(self):
        self.image_index, entries = read_image_set(self.data_path, self.image_set)
        return [{'imname': e['imname'], 'flipped': False, 'objs': e['objs'], 'shape': e['shape'],
                 'label': encode_boxes(e['objs'], e['shape'][0], e['shape'][1], self.image_size, self.cell_size)}
                for e in entries]

    def prepare(self):
        gt_labels = self.load_labels()
        if self.flipped:
            gt_labels = gt_labels + [dict(g, label=flip_label(g['label'], self.image_size), flipped=True)
                                     for g in gt_labels]
        return self._start_order(gt_labels)

    # ---- pascal_voc.py:60-67
    def image_read_u8(self, imname, flipped=False):
        img = self._cache.get(imname)
        if img is None:
            img = resize_bilinear_u8(imread_bgr(imname), self.image_size, self.image_size)
            if self.cache_images:
                self._cache[imname] = img
        return img[:, ::-1, :] if flipped else img

    def image_read(self, imname, flipped=False):
        image = self.image_read_u8(imname, flipped).astype(np.float32)
        return (image / 255.0) * 2.0 - 1.0

    def _augmented(self, g):
        """(uint8 BGR image, label grid) of entry g under the next row of the augmentation stream (img_dataset/augment.py:
        not in the reference).  The DECODED image is what is kept with cache_images: every use cuts another window.
        That is every image at native resolution in host memory, about 2.8 GB for VOC2007 trainval (5,011 images of about
        0.56 MB) against 520 KB per image of the plain cache at 416 x 416; cache_images=False decodes every time."""
        img = self._decoded.get(g['imname'])
        if img is None:
            img = imread_bgr(g['imname'])
            if self.cache_images:
                self._decoded[g['imname']] = img
        row = self.augment.draw(self.aug_rng, g['shape'][0], g['shape'][1])
        out = (self.augment.image(img, row, self.image_size, self.image_size, flip=g['flipped']),
               self.augment.label(g['objs'], row, self.image_size, self.cell_size, self.num_class, flip=g['flipped']))
        if self.max_boxes is not None:
            out += self._box_list(g, row)
        return out

    def _box_list(self, g, row=None):
        """(truth [T,5] float32, count) of entry g: every object, under the row's window (default: the whole image)"""
        from .augment import encode_box_list, identity_row
        if row is None:
            row = identity_row(g['shape'][0], g['shape'][1])
        return encode_box_list(g['objs'], row, self.image_size, self.max_boxes, flip=g['flipped'])

    # ---- pascal_voc.py:42-58 (the cursor: ShardedOrder._next)
    def get(self):
        if self.augment is not None or self.max_boxes is not None:
            images, *labels = self.get_u8()
            return ((images.astype(np.float32) / 255.0) * 2.0 - 1.0, *labels)
        images = np.zeros((self.batch_size, self.image_size, self.image_size, 3), np.float32)
        labels = np.zeros((self.batch_size, self.cell_size, self.cell_size, 25), np.float32)
        for count in range(self.batch_size):
            g = self._next()
            images[count] = self.image_read(g['imname'], g['flipped'])
            labels[count] = g['label']
        return images, labels

    def get_u8(self, images_out=None, labels_out=None):
        """the batch get() would return, images as uint8 BGR; writes into caller buffers (pinned memory) if given"""
        images = np.empty((self.batch_size, self.image_size, self.image_size, 3), np.uint8) if images_out is None \
            else images_out
        labels = np.empty((self.batch_size, self.cell_size, self.cell_size, 25), np.float32) if labels_out is None \
            else labels_out
        lists = self.max_boxes is not None
        if lists:
            truth = np.zeros((self.batch_size, self.max_boxes, 5), np.float32)
            ntruth = np.zeros(self.batch_size, np.int32)
        for count in range(self.batch_size):
            g = self._next()
            if self.augment is not None:
                images[count], labels[count], *more = self._augmented(g)
                if lists:
                    truth[count], ntruth[count] = more
                continue
            images[count] = self.image_read_u8(g['imname'], g['flipped'])
            labels[count] = g['label']
            if lists:
                truth[count], ntruth[count] = self._box_list(g)
        return (images, labels, truth, ntruth) if lists else (images, labels)
