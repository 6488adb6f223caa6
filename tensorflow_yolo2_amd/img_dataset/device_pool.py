"""The device-resident image pool that DeviceVOC (device_voc.py), DeviceCls (device_cls.py) and DeviceImages
(device_images.py) derive from, and the per-call plumbing of their batches.

Pool layout: image k starts at byte offset off[k] (a multiple of 16), rows pitch[k] = 3 * width rounded up to 16 bytes
apart, BGR uint8; the bytes between 3 * width and the pitch are zero.  Every image is decoded ONCE, at the resolution it is
stored at; no host copy is kept.  Entry table: int64 [entries][5] = {off, height, width, pitch, flip}.

DevicePool owns the construction (_build_pool: layout, the max_pool_bytes refusal, entry table, allocation, one _put per
image, the table's upload), the three places that touch device memory at start-up (_alloc_pool, _put, _upload: tests stub
them on the subclasses), the comparison of the ranks' lists, and list_batch: the entries start, start + 1, ... in LIST
order, stretched or letterboxed by one launch.  A subclass sets `entries` ([{'imname', 'shape'}, ...]), `batch_size` and
`device` before it calls _build_pool."""
import ctypes as C

import numpy as np

ALIGN = 16
DEFAULT_MAX_POOL_BYTES = 16 << 30


def _round_up(v, a):
    return (int(v) + a - 1) // a * a


def pool_layout(shapes):
    """(offsets, pitches, total bytes) of images of the given (height, width) shapes, 16-byte aligned"""
    offsets, pitches, total = [], [], 0
    for (h, w) in shapes:
        pitch = _round_up(3 * w, ALIGN)
        offsets.append(total)
        pitches.append(pitch)
        total += _round_up(h * pitch, ALIGN)
    return offsets, pitches, total


def padded_rows(img, pitch):
    """[H, W, 3] uint8 -> [H, pitch] uint8, zero bytes after 3 * W"""
    h, w = img.shape[:2]
    out = np.zeros((h, pitch), np.uint8)
    out[:, :3 * w] = img.reshape(h, 3 * w)
    return out


# ---- what every call that launches a kernel on the pool does, once
def _ptr(t):
    return C.c_void_p(t.data_ptr())


def check_size(size):
    if size < 32 or size % 32:
        raise ValueError("size %r is not a positive multiple of 32" % (size,))


def need_gpu(device, who):
    import torch
    if torch.device(device).type != "cuda":
        raise RuntimeError("%s needs the pool on the GPU (device=%r)" % (who, device))


def stream_of(tensor):
    """the handle of the current stream of the tensor's device"""
    import torch
    return C.c_void_p(torch.cuda.current_stream(tensor.device).cuda_stream)


def upload_async(tensor, array):
    """array -> device tensor from pinned memory, asynchronous on the current stream"""
    import torch
    tensor.copy_(torch.from_numpy(array).pin_memory(), non_blocking=True)


def list_index(start, batch_size, n):
    """the entries of the slots of a batch in list order: start, start + 1, ..., the final entry repeated"""
    if not 0 <= start < n:
        raise IndexError("start = %r outside the %d entries" % (start, n))
    return np.minimum(np.arange(start, start + batch_size), n - 1)


class DevicePool(object):
    def _build_pool(self, decode, max_pool_bytes):
        """pool, table, offsets, pitches, pool_bytes from self.entries; decode(k) is the image of entry k, [H, W, 3]
        uint8 BGR of the entry's shape"""
        shapes = [e['shape'] for e in self.entries]
        self.offsets, self.pitches, self.pool_bytes = pool_layout(shapes)
        if self.pool_bytes > max_pool_bytes:
            raise MemoryError("the decoded image pool needs %d bytes (%d images), max_pool_bytes is %d"
                              % (self.pool_bytes, len(self.entries), max_pool_bytes))
        table = self._entry_table()
        self.pool = self._alloc_pool(self.pool_bytes)
        for k, (e, off, pitch) in enumerate(zip(self.entries, self.offsets, self.pitches)):
            img = decode(k)
            assert img.shape == (e['shape'][0], e['shape'][1], 3), (e['imname'], img.shape, e['shape'])
            self._put(self.pool, off, padded_rows(img, pitch).reshape(-1))
        self.table = self._upload(table)
        self._eval_buffers = {}

    def _entry_table(self):
        """int64 [entries][5] = {off, height, width, pitch, 0}"""
        return np.array([(off, e['shape'][0], e['shape'][1], pitch, 0)
                         for e, off, pitch in zip(self.entries, self.offsets, self.pitches)], np.int64)

    # ---- the only places that touch device memory at start-up (torch supplies allocations and copies)
    def _alloc_pool(self, nbytes):
        import torch
        return torch.zeros(nbytes, dtype=torch.uint8, device=self.device)

    def _put(self, pool, offset, flat_u8):
        import torch
        pool[offset:offset + flat_u8.size].copy_(torch.from_numpy(flat_u8))

    def _upload(self, array):
        import torch
        return torch.from_numpy(np.ascontiguousarray(array)).to(self.device)

    def _check_ranks_agree(self):
        """stride sharding assumes ONE list on every rank: compare its length and first shuffled order (the subclass's
        order_digest)"""
        if self.world <= 1:
            return
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() == self.world):
            return                                          # plain constructor arguments, no process group
        mine = self.order_digest()
        every = [None] * self.world
        dist.all_gather_object(every, mine)
        if any(tuple(d) != tuple(mine) for d in every):
            raise RuntimeError("ranks hold different image lists or orders (entries, crc32 per rank): %r" % (every,))

    def list_batch(self, who, size, start, letterbox, fill, protocol="repo"):
        """(images [B, size, size, 3] uint8 BGR, valid): entries start .. start + B - 1 IN LIST ORDER, stretched (or
        letterboxed: the aspect ratio kept, the rest of the square `fill`) on the current stream; the last batch repeats
        its final entry and `valid` is the number of slots that are entries of their own.  Sets `eval_index`, the int32
        [B] device tensor of the slots' entries; the buffers are kept per size.  `who` names the caller in a refusal.
        protocol="darknet": the images are float32 RGB in [0, 1] instead, Darknet's letterbox_image
        (pascal_voc.letterbox_darknet; y2_letterbox_darknet_batch: one launch from the pool to the network's input), in a
        buffer of their own per size.  That protocol is letterboxed by definition and its bars are 0.5: `letterbox` and
        `fill` are not read, and a `fill` other than the default is refused."""
        import torch
        from .. import _lib
        need_gpu(self.device, who)
        check_size(size)
        if protocol == "darknet":
            return self._list_batch_darknet(size, start, fill)
        if protocol != "repo":
            raise ValueError("protocol %r is neither 'repo' nor 'darknet'" % (protocol,))
        if letterbox and not 0 <= int(fill) <= 255:
            raise ValueError("fill %r outside 0..255" % (fill,))
        n = len(self.entries)
        host = list_index(start, self.batch_size, n).astype(np.int32)
        if size not in self._eval_buffers:
            self._eval_buffers[size] = (
                torch.empty((self.batch_size, size, size, 3), dtype=torch.uint8, device=self.device),
                torch.empty(self.batch_size, dtype=torch.int32, device=self.device))
        images, index = self._eval_buffers[size]
        upload_async(index, host)
        if letterbox:
            _lib.check(_lib.load().y2_letterbox_u8_batch(_ptr(self.pool), _ptr(self.table), _ptr(index), self.batch_size,
                                                         size, int(fill), _ptr(images), stream_of(images)))
        else:
            _lib.check(_lib.load().y2_resize_bilinear_u8_batch(_ptr(self.pool), _ptr(self.table), _ptr(index),
                                                               self.batch_size, size, size, _ptr(images),
                                                               stream_of(images)))
        self.eval_index = index
        return images, min(self.batch_size, n - start)

    def _list_batch_darknet(self, size, start, fill):
        """list_batch under Darknet's protocol: the same index and last-batch rule, a float32 batch kept per size"""
        import torch
        from .. import _lib
        if fill != 127:
            raise ValueError("fill = %r with protocol='darknet': its bars are 0.5 and `fill` is not read" % (fill,))
        n = len(self.entries)
        host = list_index(start, self.batch_size, n).astype(np.int32)
        key = ("darknet", size)
        if key not in self._eval_buffers:
            self._eval_buffers[key] = (
                torch.empty((self.batch_size, size, size, 3), dtype=torch.float32, device=self.device),
                torch.empty(self.batch_size, dtype=torch.int32, device=self.device))
        images, index = self._eval_buffers[key]
        upload_async(index, host)
        _lib.check(_lib.load().y2_letterbox_darknet_batch(_ptr(self.pool), _ptr(self.table), _ptr(index), self.batch_size,
                                                          size, _ptr(images), stream_of(images)))
        self.eval_index = index
        return images, min(self.batch_size, n - start)
