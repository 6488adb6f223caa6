"""Darknet's dataset files for the YOLOv2 family (host only: numpy and the standard library): the `.data` file that names
a data set, the image list it points to, the `labels/*.txt` file that goes with every image, and the conversion of a
label file's rows to the box table's convention (img_dataset/device_voc.py).

No Darknet source or data file was at hand when this was written: the rules below are restated from memory of Darknet's
`src/option_list.c` (read_data_cfg) and `src/data.c` (get_paths, find_replace of the label path, read_boxes), as the
cfg section's are (utils/darknet_cfg.py).

`.data` grammar: `key = value` lines; blank lines and lines starting with `#` or `;` are skipped; whitespace around keys
and values is ignored; a later duplicate key wins.  Keys: `classes` (integer >= 1, required), `train`, `valid`, `names`,
`backup`, `results` (paths, kept as written) and `eval` (`voc` or `coco`, default `voc`).  Anything else -- another key, a
value that does not parse, a line that is no entry -- raises ValueError("file:line: ...") in darknet_cfg's error form: a
silently ignored key is how a run ends up reading another data set than its file says.

A label file holds one `class cx cy w h` line per object: the class index and the box's centre and extent as fractions
of the image.  to_pixel_boxes turns them into the 1-based corners of the box table (xmax - xmin is the extent), so that
the encoders give cx * size, cy * size, w * size, h * size back to within one float32 rounding (for boxes inside the
image)."""
import collections
import math
import os

# the record of one file.  train, valid, names, backup, results: paths as written, None where the key is absent
DarknetData = collections.namedtuple("DarknetData", "path classes train valid names backup results eval")

PATH_KEYS = ("train", "valid", "names", "backup", "results")
EVAL_KINDS = ("voc", "coco")
DIR_RULES = ("images", "JPEGImages", "raw")             # each replaced by "labels", first occurrence, in this order
EXTENSIONS = (".jpg", ".png", ".JPG", ".JPEG")          # the first one found becomes ".txt"


def read_data(path):
    """a .data file -> DarknetData"""
    with open(path) as f:
        text = f.read()
    entries = {}
    for no, raw in enumerate(text.splitlines(), 1):
        s = raw.strip()
        if not s or s[0] in "#;":
            continue
        if "=" not in s:
            raise ValueError("%s:%d: %r is no key = value" % (path, no, s))
        key, value = s.split("=", 1)
        key, value = key.strip(), value.strip()
        if key not in PATH_KEYS + ("classes", "eval"):
            raise ValueError("%s:%d: unknown key %s=%s" % (path, no, key, value))
        entries[key] = (value, no)
    if "classes" not in entries:
        raise ValueError("%s:%d: classes is missing" % (path, max(1, len(text.splitlines()))))
    value, no = entries["classes"]
    try:
        classes = int(value)
    except ValueError:
        raise ValueError("%s:%d: classes=%s is no integer" % (path, no, value))
    if classes < 1:
        raise ValueError("%s:%d: classes=%s: at least 1" % (path, no, value))
    kind, no = entries.get("eval", ("voc", 0))
    if kind not in EVAL_KINDS:
        raise ValueError("%s:%d: eval=%s is neither voc nor coco" % (path, no, kind))
    for key in PATH_KEYS:
        if key in entries and not entries[key][0]:
            raise ValueError("%s:%d: %s= names no path" % (path, entries[key][1], key))
    paths = {k: entries[k][0] if k in entries else None for k in PATH_KEYS}
    return DarknetData(path=path, classes=classes, eval=kind, **paths)


def read_list(path):
    """an image list -> the paths, one per non-blank line, as written (a relative one is relative to the working
    directory, as in Darknet); a path that does not exist raises, naming list:line"""
    out = []
    with open(path) as f:
        for no, raw in enumerate(f, 1):
            s = raw.strip()
            if not s:
                continue
            if not os.path.isfile(s):
                raise ValueError("%s:%d: image %s does not exist" % (path, no, s))
            out.append(s)
    return out


def label_path(image_path):
    """the label file of an image, Darknet's rule: the first `images` becomes `labels`, then the first `JPEGImages`, then
    the first `raw`, each on the result of the one before; then the first of .jpg, .png, .JPG, .JPEG becomes .txt.  A
    path that no rule changes is an error: its label file would be the image itself"""
    out = image_path
    for word in DIR_RULES:
        out = out.replace(word, "labels", 1)
    for ext in EXTENSIONS:
        if ext in out:
            out = out.replace(ext, ".txt", 1)
            break
    if out == image_path:
        raise ValueError("%s: no rule of the label path changes it (images, JPEGImages, raw -> labels; .jpg, .png, .JPG, "
                         ".JPEG -> .txt)" % image_path)
    return out


def read_labels(path, classes, image=None):
    """a label file -> [(class, cx, cy, w, h)] in file order, an empty list for an empty file.  The class is an integer of
    [0, classes), the four numbers are finite, w > 0 and h > 0; a malformed line raises, naming file:line and the item.
    A missing file raises, naming the image it belongs to (`image`)"""
    if not os.path.isfile(path):
        raise ValueError("%s: the label file of image %s does not exist" % (path, image if image is not None else "?"))
    rows = []
    with open(path) as f:
        for no, raw in enumerate(f, 1):
            parts = raw.split()
            if not parts:
                continue
            if len(parts) != 5:
                raise ValueError("%s:%d: %d values, a line is `class cx cy w h`" % (path, no, len(parts)))
            try:
                cls = int(parts[0])
            except ValueError:
                raise ValueError("%s:%d: class %s is no integer" % (path, no, parts[0]))
            if not 0 <= cls < classes:
                raise ValueError("%s:%d: class %d outside 0..%d" % (path, no, cls, classes - 1))
            box = []
            for name, word in zip(("cx", "cy", "w", "h"), parts[1:]):
                try:
                    v = float(word)
                except ValueError:
                    raise ValueError("%s:%d: %s=%s is no number" % (path, no, name, word))
                if not math.isfinite(v):
                    raise ValueError("%s:%d: %s=%s is not finite" % (path, no, name, word))
                box.append(v)
            for name, v in (("w", box[2]), ("h", box[3])):
                if not v > 0:
                    raise ValueError("%s:%d: %s=%r must be positive" % (path, no, name, v))
            rows.append((cls,) + tuple(box))
    return rows


def to_pixel_boxes(rows, height, width):
    """label rows -> the box table's objects [(xmin, ymin, xmax, ymax, class)]: 1-based corners whose difference is the
    extent, xmin = (cx - w / 2) * W + 1, xmax = (cx + w / 2) * W + 1 and the same in y, every operation rounded on its
    own in float64.  height, width: the DECODED image's"""
    W, H = float(width), float(height)
    out = []
    for (cls, cx, cy, w, h) in rows:
        cx, cy, w, h = float(cx), float(cy), float(w), float(h)
        hw, hh = w / 2.0, h / 2.0
        out.append(((cx - hw) * W + 1.0, (cy - hh) * H + 1.0, (cx + hw) * W + 1.0, (cy + hh) * H + 1.0, int(cls)))
    return out


def from_pixel_boxes(objs, height, width):
    """the inverse of to_pixel_boxes: box-table objects -> label rows (a devkit converted to label files)"""
    W, H = float(width), float(height)
    out = []
    for (xmin, ymin, xmax, ymax, cls) in objs:
        x1, y1, x2, y2 = float(xmin) - 1.0, float(ymin) - 1.0, float(xmax) - 1.0, float(ymax) - 1.0
        out.append((int(cls), (x1 + x2) / 2.0 / W, (y1 + y2) / 2.0 / H, (x2 - x1) / W, (y2 - y1) / H))
    return out


def write_labels(path, rows):
    """label rows -> a label file that read_labels reads back to the same float64 values (repr round-trips); the
    directory is made where it is missing"""
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "w") as f:
        for (cls, cx, cy, w, h) in rows:
            f.write("%d %r %r %r %r\n" % (int(cls), float(cx), float(cy), float(w), float(h)))
    return path


def image_entries(list_path, classes, labels=True):
    """the pool entries of an image list: [{'imname', 'shape': (height, width), 'objs', 'difficult'}] in list order, the
    shape from the image's header, the objects from its label file.  An image whose label file is empty stays, with no
    object (Darknet's negatives); `difficult` is all zero.  labels=False: no label file is read and no entry has an
    object -- a list that is only detected on, as Darknet's `valid` reads it"""
    from PIL import Image
    entries = []
    for imname in read_list(list_path):
        with Image.open(imname) as im:
            w, h = im.size
        objs = to_pixel_boxes(read_labels(label_path(imname), classes, image=imname), h, w) if labels else []
        entries.append({'imname': imname, 'shape': (int(h), int(w)), 'objs': objs, 'difficult': [0] * len(objs)})
    return entries


def image_id_of(image_path):
    """the COCO image id of a path as Darknet's `valid` takes it: the digits of the file name after its last `_` (the
    whole stem where there is none), COCO_val2014_000000000139.jpg -> 139"""
    stem = os.path.splitext(os.path.basename(image_path))[0]
    digits = "".join(c for c in stem.rsplit("_", 1)[-1] if c.isdigit())
    if not digits:
        raise ValueError("%s: no digits in the file name to take a COCO image id from" % image_path)
    return int(digits)


COCO_IDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 27, 28, 31, 32, 33, 34, 35,
            36, 37, 38, 39, 40, 41, 42, 43, 44, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64,
            65, 67, 70, 72, 73, 74, 75, 76, 77, 78, 79, 80, 81, 82, 84, 85, 86, 87, 88, 89, 90)


def coco_category_ids(classes):
    """the category id a results file names class c by: COCO's 80 published ids (the order of coco.names) for an
    80-class model, else c + 1"""
    return list(COCO_IDS) if classes == len(COCO_IDS) else list(range(1, classes + 1))
