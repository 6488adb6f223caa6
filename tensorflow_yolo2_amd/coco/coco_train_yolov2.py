"""Train the YOLOv2 anchor detector on the images of a COCO instances file (not in the reference):
    python -m tensorflow_yolo2_amd.coco.coco_train_yolov2 --annotations instances_train2014.json --images train2014 \
        [--image-list trainvalno5k.txt] --cfg yolov2.cfg --darknet-backbone darknet19_448.conv.23 --ckpt-dir backup \
        [--max-pool-bytes BYTES] [every flag of pascal_train_yolov2 but --devkit]
The trainer is pascal_train_yolov2's, through its data-set seam: the pool is DeviceCOCOTrain (img_dataset/device_coco.py)
-- the file's images in ascending id, crowd annotations and boxes without extent left out, images without objects kept as
negatives -- and the draw is on (--draw-boxes): COCO images often hold more than --max-boxes objects, and such an image
trains a subset drawn anew at every use, as in Darknet.  The model's class count (the cfg's) must be the file's category
count.

The pool is decoded once, at native resolution: train2014 + val2014 minus the 5k (117,264 images of about 640 x 480 x 3 =
0.9 MB) is about 108 GB, so --max-pool-bytes has to be raised well above the 16 GB default, and the device has to hold it."""
import sys

from ..img_dataset.device_pool import DEFAULT_MAX_POOL_BYTES
from ..pascal import pascal_train_yolov2 as T

PROG = "python -m tensorflow_yolo2_amd.coco.coco_train_yolov2"
OWN_FLAGS = {"--annotations": None, "--images": None, "--image-list": None, "--max-pool-bytes": None}


def split_args(argv):
    """(this script's own flags as a dict, the rest for pascal_train_yolov2.parse_args); `--flag value` and `--flag=value`"""
    own, rest, k = dict(OWN_FLAGS), [], 0
    while k < len(argv):
        word = argv[k]
        flag, eq, value = word.partition("=")
        if flag in own:
            if not eq:
                k += 1
                if k >= len(argv):
                    raise ValueError("%s needs a value" % flag)
                value = argv[k]
            own[flag] = value
        else:
            rest.append(word)
        k += 1
    return own, rest


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    try:
        own, rest = split_args(argv)
    except ValueError as e:
        sys.exit("%s: error: %s" % (PROG, e))
    args = T.parse_args(rest, need_devkit=False, prog=PROG + " --annotations FILE --images DIR [--image-list FILE] "
                        "[--max-pool-bytes BYTES]", draw_boxes=True)
    if own["--annotations"] is None or own["--images"] is None:
        args.error("--annotations FILE and --images DIR are needed")
    try:
        max_pool_bytes = DEFAULT_MAX_POOL_BYTES if own["--max-pool-bytes"] is None else int(own["--max-pool-bytes"])
    except ValueError:
        args.error("--max-pool-bytes %s is no integer" % own["--max-pool-bytes"])
    args.dataset_name = own["--annotations"]

    def dataset(a):
        from ..img_dataset.device_coco import DeviceCOCOTrain
        try:
            return DeviceCOCOTrain(own["--annotations"], own["--images"], a.batch, image_list=own["--image-list"],
                                   flipped=a.flipped, seed=a.seed, max_pool_bytes=max_pool_bytes, augment=a.augmentation,
                                   max_boxes=a.max_boxes if a.box_labels else None, draw=a.draw_boxes)
        except (OSError, ValueError) as e:
            a.error("--annotations: %s" % e)
    return T.main(args, dataset=dataset)


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
