"""A device-resident pool of plain image files: the pool and the entry table of DeviceVOC (device_voc.py: same layout,
same kernels) built from a list of paths, without a devkit and without annotations -- what the anchor detector needs to
run on an image that is not part of VOC (pascal/pascal_detect_yolov2.py).

Every file is decoded ONCE into the uint8 pool at its native resolution (pool_layout, padded_rows, imread_bgr); the entry
table is int64 [entries][5] = {off, height, width, pitch, 0}.  build_tables needs object lists, so the table is made here
and there is no box table.  batch(size, start, letterbox=True) has DeviceVOC.eval_batch's contract: the entries start,
start + 1, ... in list order, letterboxed (or, with letterbox=False, stretched) to size x size on the current stream, the
last batch filled with its final entry, `eval_index` the int32 [B] device tensor of the slots' entries."""
import numpy as np

from .device_voc import DEFAULT_MAX_POOL_BYTES, list_batch, padded_rows, pool_layout
from .pascal_voc import imread_bgr


class DeviceImages(object):
    def __init__(self, paths, batch_size, device="cuda", max_pool_bytes=DEFAULT_MAX_POOL_BYTES):
        self.paths = [str(p) for p in paths]
        if not self.paths:
            raise ValueError("DeviceImages needs at least one image file")
        if int(batch_size) < 1:
            raise ValueError("batch_size %r must be at least 1" % (batch_size,))
        self.batch_size, self.device = int(batch_size), device
        images = [imread_bgr(p) for p in self.paths]
        self.entries = [{'imname': p, 'shape': img.shape[:2]} for p, img in zip(self.paths, images)]
        self.offsets, self.pitches, self.pool_bytes = pool_layout([e['shape'] for e in self.entries])
        if self.pool_bytes > max_pool_bytes:
            raise MemoryError("the decoded image pool needs %d bytes (%d images), max_pool_bytes is %d"
                              % (self.pool_bytes, len(self.entries), max_pool_bytes))
        table = np.array([(off, e['shape'][0], e['shape'][1], pitch, 0)
                          for e, off, pitch in zip(self.entries, self.offsets, self.pitches)], np.int64)
        self.pool = self._alloc_pool(self.pool_bytes)
        for img, off, pitch in zip(images, self.offsets, self.pitches):
            self._put(self.pool, off, padded_rows(img, pitch).reshape(-1))
        self.table = self._upload(table)
        self._eval_buffers = {}

    # ---- the only places that touch device memory at start-up, as in DeviceVOC
    def _alloc_pool(self, nbytes):
        import torch
        return torch.zeros(nbytes, dtype=torch.uint8, device=self.device)

    def _put(self, pool, offset, flat_u8):
        import torch
        pool[offset:offset + flat_u8.size].copy_(torch.from_numpy(flat_u8))

    def _upload(self, array):
        import torch
        return torch.from_numpy(np.ascontiguousarray(array)).to(self.device)

    def batch(self, size, start, letterbox=True, fill=127):
        """(images [B, size, size, 3] uint8 BGR, valid) of the entries start .. start + B - 1: DeviceVOC.eval_batch"""
        return list_batch(self, "DeviceImages.batch", size, start, letterbox, fill)
