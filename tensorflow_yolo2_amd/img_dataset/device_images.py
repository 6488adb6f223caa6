"""A device-resident pool of plain image files: the pool, the entry table and the list-order batches of DevicePool
(device_pool.py) built from a list of paths, without a devkit and without annotations -- what the anchor detector needs
to run on an image that is not part of VOC (pascal/pascal_detect_yolov2.py).

Every file is decoded ONCE into the uint8 pool at its native resolution; the entry table is the plain one, int64
[entries][5] = {off, height, width, pitch, 0}, and there is no box table.  batch(size, start, letterbox=True) has
DeviceVOC.eval_batch's contract: the entries start, start + 1, ... in list order, letterboxed (or, with letterbox=False,
stretched) to size x size on the current stream, the last batch filled with its final entry, `eval_index` the int32 [B]
device tensor of the slots' entries."""
from .device_pool import DEFAULT_MAX_POOL_BYTES, DevicePool
from .pascal_voc import imread_bgr


class DeviceImages(DevicePool):
    def __init__(self, paths, batch_size, device="cuda", max_pool_bytes=DEFAULT_MAX_POOL_BYTES):
        self.paths = [str(p) for p in paths]
        if not self.paths:
            raise ValueError("DeviceImages needs at least one image file")
        if int(batch_size) < 1:
            raise ValueError("batch_size %r must be at least 1" % (batch_size,))
        self.batch_size, self.device = int(batch_size), device
        images = [imread_bgr(p) for p in self.paths]
        self.entries = [{'imname': p, 'shape': img.shape[:2]} for p, img in zip(self.paths, images)]
        self._build_pool(images.__getitem__, max_pool_bytes)

    def batch(self, size, start, letterbox=True, fill=127, protocol="repo"):
        """(images [B, size, size, 3] uint8 BGR, valid) of the entries start .. start + B - 1: DeviceVOC.eval_batch"""
        return self.list_batch("DeviceImages.batch", size, start, letterbox, fill, protocol)
