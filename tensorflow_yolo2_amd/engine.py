"""Host-side driver of one network context of libyolo2_hip.so.

PyTorch is plumbing only: it owns device memory (flat parameter / gradient /
BN-state buffers, one workspace blob) and the HIP stream handle.  Every
computation is a hand-written gfx950 kernel behind the C ABI; nothing here
falls back to torch ops.

Reference counterpart: the TF1 graph + variables that
src/yolo2_nets/darknet.py builds, and the autodiff graph of
src/pascal/pascal_train_darknet.py:49-51.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import check

# (filter_size, in_chl, out_chl, maxpool_after) -- src/yolo2_nets/darknet.py:150-177
CORE_SPEC = [
    (3, 3, 32, 1),
    (3, 32, 64, 1),
    (3, 64, 128, 0), (3, 128, 64, 0), (3, 64, 128, 1),
    (3, 128, 256, 0), (1, 256, 128, 0), (3, 128, 256, 1),
    (3, 256, 512, 0), (1, 512, 256, 0), (3, 256, 512, 0), (1, 512, 256, 0), (3, 256, 512, 1),
    (3, 512, 1024, 0), (1, 1024, 512, 0), (3, 512, 1024, 0), (1, 1024, 512, 0), (3, 512, 1024, 0),
]


def det_head_spec(output_filter):
    """src/yolo2_nets/darknet.py:189-200."""
    return [(3, 1024, 1024, 0)] * 3 + [(1, 1024, output_filter, 0)]


CLS_HEAD_SPEC = [(1, 1024, 1000, 0)]   # src/yolo2_nets/darknet.py:115

PARAM_KEYS = ("W", "b", "gamma", "beta")
STATE_KEYS = ("moving_mean", "moving_var")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- the tensor contracts of the entry points below, each stated once.  Plain functions with positional arguments:
# several of them front kernels of about 10 us, where a Python frame shows (docs/HISTORY.md), so nothing here builds a
# closure, a dict or a format string on the success path, and the callers pass the counts they already hold.
def _dev(t, dtype, name):
    """t is a contiguous device tensor of dtype"""
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous(), name
    return t


def _chk(*ts):
    """contiguous fp32 device tensors, or None"""
    for t in ts:
        if t is not None:
            _dev(t, torch.float32, "operand")


def _entries(table, index, n, rows):
    """the entries of a batch of n: table int64 [entries][5] (DeviceVOC.table; None where a call has no table), and
    index int32 [at least n] on the device, or None for the first n of `rows` entries"""
    if table is not None:
        assert table.is_cuda and table.dtype == torch.int64 and table.is_contiguous() and table.shape[-1] == 5, "table"
    if index is not None:
        assert index.is_cuda and index.dtype == torch.int32 and index.is_contiguous() and index.numel() >= n, "index"
    else:
        assert rows >= n, (rows, n)


def _upload_anchors(anchors, device):
    """anything numpy reads -> a contiguous float32 tensor on the device"""
    return torch.as_tensor(np.asarray(anchors, np.float32)).to(device).contiguous()


def _anchors(anchors, B, device):
    """anchors [B,2]: a float32 device tensor as it is, or anything numpy reads, uploaded"""
    if torch.is_tensor(anchors):
        an = anchors
        assert an.is_cuda and an.dtype == torch.float32 and an.is_contiguous(), "anchors"
    else:
        an = _upload_anchors(anchors, device)
    assert an.numel() == 2 * B, (tuple(an.shape), B)
    return an


def _own(t, shape, dtype, device, numel=None):
    """an output tensor of `shape`: allocated when t is None, else the caller's own device tensor, contiguous and of
    dtype, of exactly that shape -- or, with numel, of that element count (callers pass views of another shape)"""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous(), "out"
    if numel is None:
        assert tuple(t.shape) == tuple(shape), t.shape
    else:
        assert t.numel() == numel, t.shape
    return t


def _det_out(out, lead, segments, m, device):
    """the (det int32 lead + [m,6], score float32 lead + [m], count int32 lead) of a detect call over `segments` =
    prod(lead) images or (image, class) pairs: allocated, or the caller's `out` checked by element count (callers pass
    views such as det.view(n * C, m, 6)); where the caller's tensors live is not checked"""
    if out is None:
        return (torch.empty(lead + (m, 6), dtype=torch.int32, device=device),
                torch.empty(lead + (m,), dtype=torch.float32, device=device),
                torch.empty(lead, dtype=torch.int32, device=device))
    det, score, count = out
    assert det.is_contiguous() and det.dtype == torch.int32 and det.numel() == segments * m * 6
    assert score.is_contiguous() and score.dtype == torch.float32 and score.numel() == segments * m
    assert count.is_contiguous() and count.dtype == torch.int32 and count.numel() == segments
    return det, score, count


class ForwardGraph:
    """Network.forward captured into a HIP graph (Network.forward_graph)."""

    def __init__(self, net, is_training_core, is_training_head, uint8):
        self.net = net
        shape = (net.batch, net.height, net.width, net.spec[0][1])
        self.input = torch.zeros(shape, dtype=torch.uint8 if uint8 else torch.float32, device=net.device)
        self.output = torch.empty(net.out_shape, dtype=torch.float32, device=net.device)
        self._stream = torch.cuda.Stream(device=net.device)
        self._stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._stream):
            for _ in range(2):
                net.forward(self.input, is_training_core, is_training_head, out=self.output, update_moving=False)
        self._stream.synchronize()
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph, stream=self._stream):
            net.forward(self.input, is_training_core, is_training_head, out=self.output, update_moving=False)
        self._modes = (is_training_core, is_training_head)
        self._gen = net._host_param_gen

    def replay(self):
        # load_params / init_params / params_changed re-pack the filters at the NEXT eager forward, outside any graph
        # (a replay silently ran the packs baked in at capture time).  One eager forward on the capture
        # stream brings the packed copies the graph reads up to date; the fused optimizer steps re-pack on the device
        # into those same buffers and need nothing.
        if self.net._host_param_gen != self._gen:
            self._stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self._stream):
                self.net.forward(self.input, self._modes[0], self._modes[1], out=self.output, update_moving=False)
            torch.cuda.current_stream().wait_stream(self._stream)
            self._gen = self.net._host_param_gen
        self._graph.replay()
        return self.output

    def __call__(self, images):
        self.input.copy_(images, non_blocking=True)
        return self.replay()


class Network:
    """One conv-BN-leaky(-pool) stack bound to device buffers."""

    def __init__(self, spec, batch, height, width, dtype="f16", core_layers=None, tail=_lib.Y2_TAIL_NONE,
                 tail_k=7, training=True, device="cuda:0", grad_scale=None, bessel=False, share_with=None,
                 buffers=None):
        self.lib = _lib.load()
        self._host_param_gen = 0        # bumped whenever the parameters change on a path that re-packs at the next forward
        if not torch.cuda.is_available():
            raise _lib.Y2Error("no MI355X visible: tensorflow_yolo2_amd has no CPU path")
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.spec = [tuple(int(v) for v in s) for s in spec]
        self.dtype = _lib.DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
        self.training = bool(training)
        if self.dtype == _lib.Y2_FP8 and self.training:
            raise _lib.Y2Error("dtype 'fp8' (MXFP8) is inference only: create the Network with training=False")
        self.batch, self.height, self.width = batch, height, width
        self.core_layers = len(spec) if core_layers is None else core_layers
        flat = (C.c_int * (4 * len(spec)))(*[v for s in self.spec for v in s])
        h = C.c_void_p()
        check(self.lib.y2_ctx_create(C.byref(h), flat, len(spec), self.core_layers, tail, tail_k,
                                     batch, height, width, self.dtype))
        self.h = h
        self.num_layers = len(spec)
        self.n_params = self.lib.y2_param_count(h)
        self.n_state = self.lib.y2_state_count(h)
        shp = (C.c_int * 4)()
        check(self.lib.y2_output_shape(h, shp))
        self.out_shape = tuple(shp)
        if tail == _lib.Y2_TAIL_AVGPOOL:
            self.out_shape = (shp[0], shp[3]) if shp[1] == 1 and shp[2] == 1 else tuple(shp)
        if share_with is not None:
            # same layers at another input size (the net is fully convolutional): ONE set of parameters,
            # gradients and BN state, one workspace per size (multi-scale training, 288 GB of HBM to spend)
            assert share_with.n_params == self.n_params and share_with.n_state == self.n_state
            self.params, self.grads, self.state = share_with.params, share_with.grads, share_with.state
            assert not training or self.grads is not None
        elif buffers is not None:
            # caller-owned flat buffers (a variable scope's store, yolo2_nets/darknet.py): exact-size views
            self.params, self.grads, self.state = self._check_buffers(*buffers)
        else:
            self.params = torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
            self.grads = torch.zeros(self.n_params, dtype=torch.float32, device=self.device) if training else None
            self.state = torch.zeros(self.n_state, dtype=torch.float32, device=self.device)
        self.ws_bytes = self.lib.y2_workspace_bytes(h, int(training))
        self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.device)
        check(self.lib.y2_bind(h, _ptr(self.params), _ptr(self.grads), _ptr(self.state), _ptr(self.workspace),
                               self.ws_bytes, int(training), _stream()))
        self.scale_owner = share_with.scale_owner if share_with is not None else self
        if grad_scale is None:
            # f16 and the split-operand mode (f16 planes): gradients ride on a loss scale, dY's exponent range is f16's
            grad_scale = 1024.0 if self.dtype in _lib.LOSS_SCALED else 1.0
        self.grad_scale = float(grad_scale)
        self.bn_eps, self.bn_momentum, self.zero_bias_grad = 1e-3, 0.99, False     # y2_ctx defaults (darknet.py:39-44)
        self.slopes = None         # the per-layer slopes last given to set_layer_options (None: 0.1 everywhere)
        self._bessel = bool(bessel)
        check(self.lib.y2_set_options(h, self.grad_scale, int(bessel)))
        self._offsets = []
        off = (C.c_size_t * 6)()
        for l in range(self.num_layers):
            check(self.lib.y2_param_offsets(h, l, off))
            self._offsets.append(tuple(off))
        self._out = torch.empty(self.out_shape, dtype=torch.float32, device=self.device)
        self.store = None          # yolo2_nets.darknet._VarStore when a variable scope owns the buffers

    def _check_buffers(self, params, grads, state):
        for t, n, need in ((params, self.n_params, True), (grads, self.n_params, self.training),
                           (state, self.n_state, True)):
            if t is None:
                if need:
                    raise ValueError("missing flat buffer")
                continue
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n):
                raise ValueError("flat buffer must be a contiguous float32 device tensor of %d elements" % n)
        return params, (grads if self.training else None), state

    def rebind(self, params, grads, state):
        """move this context onto other flat buffers (same sizes); the workspace is re-zeroed"""
        self.params, self.grads, self.state = self._check_buffers(params, grads, state)
        check(self.lib.y2_bind(self.h, _ptr(self.params), _ptr(self.grads), _ptr(self.state), _ptr(self.workspace),
                               self.ws_bytes, int(self.training), _stream()))

    def set_layer_options(self, slopes=None, bn_eps=None, bn_momentum=None, zero_bias_grad=None):
        """per-layer activation slopes (0.1 leaky = the reference, 0 ReLU, 1 none) and the stack's batch-norm constants
        (y2_set_layer_options).  Every argument left at None KEEPS the context's current value (a fresh context holds
        tf.layers.batch_normalization's defaults: eps 1e-3, momentum 0.99, conv biases trainable) -- a call that only
        changes the slopes does not reset a ResNet stack's eps 1e-5 / momentum 0.997."""
        arr = None
        if slopes is not None:
            assert len(slopes) == self.num_layers
            arr = (C.c_float * self.num_layers)(*[float(v) for v in slopes])
            self.slopes = [float(v) for v in slopes]
        if bn_eps is not None:
            self.bn_eps = float(bn_eps)
        if bn_momentum is not None:
            self.bn_momentum = float(bn_momentum)
        if zero_bias_grad is not None:
            self.zero_bias_grad = bool(zero_bias_grad)
        check(self.lib.y2_set_layer_options(self.h, arr, self.num_layers, self.bn_eps, self.bn_momentum,
                                            int(self.zero_bias_grad)))

    def set_grad_scale(self, grad_scale):
        self.grad_scale = float(grad_scale)
        check(self.lib.y2_set_options(self.h, self.grad_scale, int(self._bessel)))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.y2_ctx_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ---- parameters ------------------------------------------------------
    def _shapes(self, l):
        k, ci, co, _ = self.spec[l]
        return {"W": (k, k, ci, co), "b": (co,), "gamma": (co,), "beta": (co,),
                "moving_mean": (co,), "moving_var": (co,)}

    def layer_views(self, l, grads=False):
        """dict of views into the flat buffers (reference creation order W, b, gamma, beta)."""
        o = self._offsets[l]
        shp = self._shapes(l)
        src = self.grads if grads else self.params
        out = {}
        for i, k in enumerate(PARAM_KEYS):
            n = int(np.prod(shp[k]))
            out[k] = src[o[i]:o[i] + n].view(shp[k])
        if not grads:
            for i, k in enumerate(STATE_KEYS):
                n = int(np.prod(shp[k]))
                out[k] = self.state[o[4 + i]:o[4 + i] + n].view(shp[k])
        return out

    def init_params(self, seed=0):
        """darknet.py:10-17 initial values, generated on the device."""
        check(self.lib.y2_init_params(self.h, seed, _stream()))
        self._host_param_gen += 1

    def load_params(self, layers):
        """layers: list of dicts with numpy arrays W, b, gamma, beta, moving_mean, moving_var."""
        assert len(layers) == self.num_layers
        for l, p in enumerate(layers):
            v = self.layer_views(l)
            for k in PARAM_KEYS + STATE_KEYS:
                v[k].copy_(torch.as_tensor(np.asarray(p[k], np.float32)).to(self.device))
        check(self.lib.y2_params_changed(self.h))
        self._host_param_gen += 1
        if self.store is not None:
            self.store.version += 1

    def export_params(self):
        out = []
        for l in range(self.num_layers):
            out.append({k: v.detach().cpu().numpy().copy() for k, v in self.layer_views(l).items()})
        return out

    def export_grads(self):
        return [{k: v.detach().cpu().numpy().copy() for k, v in self.layer_views(l, grads=True).items()}
                for l in range(self.num_layers)]

    def params_changed(self):
        check(self.lib.y2_params_changed(self.h))
        self._host_param_gen += 1

    # ---- execution -------------------------------------------------------
    def forward(self, images, is_training_core=True, is_training_head=True, out=None, update_moving=False, join=None):
        """images: float32 NHWC in [-1, 1) (the reference's placeholder), or uint8 NHWC BGR pixels.
        join (fp32, the output's shape): the stack is the residual branch of a bottleneck unit and the result is
        relu(join + stack(images)) (slim_dir/nets/resnet_v1.py:112), written by the last layer's apply pass.
        update_moving: fold the BN moving-statistics update of the training-mode layers into this pass
        (the train step: UPDATE_OPS under train_op, pascal_train_darknet.py:49-51); False leaves them alone,
        as a sess.run that fetches only the output or the loss does (update_moving_stats() applies it later)."""
        assert images.is_cuda and images.is_contiguous() and images.dtype in (torch.float32, torch.uint8)
        assert tuple(images.shape[:3]) == (self.batch, self.height, self.width), images.shape
        out = self._out if out is None else out
        # uint8 BGR pixels (what cv2.imread + cv2.resize hand to image_read, pascal_voc.py:60-62): the conversion
        # x / 255 * 2 - 1 runs in the input pack kernel
        if join is not None:
            assert images.dtype == torch.float32 and join.is_cuda and join.dtype == torch.float32 and join.is_contiguous()
            assert join.numel() == out.numel() and join.data_ptr() != out.data_ptr()
            check(self.lib.y2_forward_join(self.h, _ptr(images), _ptr(join), int(bool(is_training_core)),
                                           int(bool(is_training_head)), int(bool(update_moving)), _ptr(out), _stream()))
            return out
        fwd = self.lib.y2_forward_u8 if images.dtype == torch.uint8 else self.lib.y2_forward
        check(fwd(self.h, _ptr(images), int(bool(is_training_core)), int(bool(is_training_head)),
                  int(bool(update_moving)), _ptr(out), _stream()))
        return out

    def forward_graph(self, is_training_core=False, is_training_head=True, uint8=False):
        """The forward pass as ONE HIP graph (serving: single-image detection is launch-bound -- ~40 kernels of 3-8 us
        behind ~4 us of host work each; a replay is one host call).  Returns a ForwardGraph: write the batch into
        `.input` (float32 NHWC, or uint8 BGR with uint8=True), call `.replay()`, read `.output` ([N,S,S,C] fp32; valid
        after a synchronisation of the current stream).  Two eager passes run first on the capture stream (filter packs,
        kernel attributes: neither may happen inside a capture).  The moving statistics are never updated by a replay.
        After a later load_params / init_params / params_changed the next replay first refreshes the packed filters
        with one eager forward (ForwardGraph.replay)."""
        return ForwardGraph(self, is_training_core, is_training_head, uint8)

    def update_moving_stats(self):
        check(self.lib.y2_update_moving_stats(self.h, _stream()))

    def backward(self, dout, layer_lo=0, layer_hi=None):
        layer_hi = self.num_layers if layer_hi is None else layer_hi
        if dout is not None:
            assert dout.is_cuda and dout.dtype == torch.float32 and dout.is_contiguous()
        check(self.lib.y2_backward(self.h, _ptr(dout), layer_lo, layer_hi, _stream()))

    # ---- linked stacks (y2_link: bottleneck units chained in the arithmetic type) -----------------------------
    def link(self, x=None, out=None, join=None, join_self=False, dout=None, dx=None):
        """tensors of the next forward / backward calls of this context: x / out / join are Bordered tensors, dout / dx
        [M][C] tensors of the arithmetic type (include/yolo2_hip.h y2_link); all None restores the fp32 interface"""
        cell = lambda b: None if b is None else C.c_void_p(b.cell0)
        raw = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        self._linked = (x, out, join, dout, dx)           # keep the tensors alive
        check(self.lib.y2_link(self.h, cell(x), cell(out), cell(join), int(bool(join_self)), raw(dout), raw(dx)))

    def forward_linked(self, is_training=True, update_moving=False, out=None, images=None):
        """forward with the linked tensors: `images` only when layer 0 is not linked, `out` (fp32) only when the output
        is not"""
        check(self.lib.y2_forward(self.h, _ptr(images) if images is not None else None, int(bool(is_training)),
                                  int(bool(is_training)), int(bool(update_moving)),
                                  _ptr(out) if out is not None else None, _stream()))
        return out

    def backward_linked(self, dout=None, dinput=None):
        """backward; dout (fp32) only when no typed output gradient is linked; dinput: fp32 [N,H,W,cin] to receive the
        input gradient as well (y2_backward_input)"""
        if dinput is not None:
            check(self.lib.y2_backward_input(self.h, _ptr(dout) if dout is not None else None, _ptr(dinput), _stream()))
        else:
            check(self.lib.y2_backward(self.h, _ptr(dout) if dout is not None else None, 0, self.num_layers, _stream()))

    def backward_input(self, dout):
        """full backward; also returns d loss / d input of the stack, fp32 [N,H,W,cin] (composed graphs)"""
        assert dout.is_cuda and dout.dtype == torch.float32 and dout.is_contiguous()
        dx = torch.empty((self.batch, self.height, self.width, self.spec[0][1]), dtype=torch.float32, device=self.device)
        check(self.lib.y2_backward_input(self.h, _ptr(dout), _ptr(dx), _stream()))
        return dx

    PROFILE_CATEGORIES = ("conv_fwd", "conv1_fwd", "dgrad", "wgrad", "conv1_wgrad", "bn_fwd", "bn_bwd", "misc")

    def backward_marks(self, dout, mark_layers):
        """full backward; mark k fires when every layer >= mark_layers[k] is complete (see wait_mark)"""
        assert dout.is_cuda and dout.dtype == torch.float32 and dout.is_contiguous()
        marks = (C.c_int * len(mark_layers))(*[int(v) for v in mark_layers])
        check(self.lib.y2_backward_marks(self.h, _ptr(dout), len(mark_layers), marks, _stream()))

    def wait_mark(self, k, stream):
        """make `stream` (a torch.cuda.Stream) wait until mark k of the last backward_marks has fired"""
        check(self.lib.y2_wait_mark(self.h, int(k), C.c_void_p(stream.cuda_stream)))

    def profile_enable(self, on=1):
        """0 off; 1 bracket every launch with HIP events (serialised: no side stream); 2 only the MFMA convolution
        launches (forward, dgrad, wgrad), streams as in production"""
        check(self.lib.y2_profile_enable(self.h, int(on)))

    def profile_busy(self, categories=("conv_fwd", "dgrad", "wgrad")):
        """(busy milliseconds, launches): union of the intervals of those launch categories (call before collect)"""
        mask = sum(1 << self.PROFILE_CATEGORIES.index(k) for k in categories)
        ms, n = C.c_double(), C.c_int()
        check(self.lib.y2_profile_busy(self.h, mask, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_layers(self):
        """[num_layers][8] milliseconds per layer and category of the records so far (call before collect)"""
        buf = (C.c_double * (self.num_layers * len(self.PROFILE_CATEGORIES)))()
        check(self.lib.y2_profile_layers(self.h, buf))
        return np.array(buf).reshape(self.num_layers, len(self.PROFILE_CATEGORIES))

    def profile_collect(self):
        n = len(self.PROFILE_CATEGORIES)
        ms = (C.c_double * n)()
        cnt = (C.c_int * n)()
        check(self.lib.y2_profile_collect(self.h, ms, cnt, n))
        return {k: (ms[i], cnt[i]) for i, k in enumerate(self.PROFILE_CATEGORIES)}

    def layer_statistics(self, layer):
        """the per-channel constants the last forward normalised `layer` with (y2_debug_read selector 3): dict of float64
        arrays mean, invstd, scale, shift and var = 1 / invstd^2 - eps (the biased batch variance, or the moving one)"""
        co = self.spec[layer][2]
        t = torch.empty((4, co), dtype=torch.float32, device=self.device)
        check(self.lib.y2_debug_read(self.h, layer, 3, _ptr(t), _stream()))
        a = t.double().cpu().numpy()
        eps = self.bn_eps
        return {"mean": a[0], "invstd": a[1], "scale": a[2], "shift": a[3], "var": 1.0 / (a[1] * a[1]) - eps}

    def debug_read(self, layer, what):
        k, ci, co, _ = self.spec[layer]
        info = (C.c_int * 8)()
        check(self.lib.y2_layer_info(self.h, layer, info))
        c = ci if what == 0 else co
        t = torch.empty((self.batch, info[4], info[5], c), dtype=torch.float32, device=self.device)
        check(self.lib.y2_debug_read(self.h, layer, what, _ptr(t), _stream()))
        return t


class Bordered:
    """a zero-bordered activation tensor [N][H+1][W+1][C] of the arithmetic type with its guard bands (csrc/common.h
    bpix), allocated zeroed once: what two linked stacks share (Network.link)"""

    def __init__(self, n, h, w, c, dtype, device):
        lib = _lib.load()
        dt = _lib.DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
        if dt not in (_lib.Y2_F32, _lib.Y2_F16, _lib.Y2_BF16):
            # (the type map below has no entry for the split-operand modes, whose cells are two half planes;
            #  y2_link refuses them too)
            raise ValueError("Bordered: linked tensors exist in f32 / f16 / bf16 (not the split-operand modes f16x2 / f16x2f)")
        off = C.c_size_t(0)
        nbytes = lib.y2_bordered_bytes(n, h, w, c, dt, C.byref(off))
        self.buf = torch.zeros(nbytes, dtype=torch.uint8, device=device)
        self.cell0 = self.buf.data_ptr() + off.value
        self.shape = (n, h, w, c)
        self._off, self._tdtype = off.value, {_lib.Y2_F32: torch.float32, _lib.Y2_F16: torch.float16, _lib.Y2_BF16: torch.bfloat16}[dt]

    def _interior(self):
        """view of the image cells [N, H, W, C] in the tensor's own type: cell (n, h, w) sits at row n (H + 1) + h + 1,
        column w + 1 of a (W + 1)-wide pixel grid that starts at cell 0"""
        n, h, w, c = self.shape
        esz = torch.empty(0, dtype=self._tdtype).element_size()
        rows = n * (h + 1)
        body = self.buf[self._off:self._off + rows * (w + 1) * c * esz].view(self._tdtype).view(n, h + 1, w + 1, c)
        return body[:, 1:, 1:, :]

    def write(self, x):
        """tests: fill the image cells from an fp32 NHWC tensor (borders stay zero)"""
        self._interior().copy_(x.to(self._tdtype))

    def read(self):
        return self._interior().float()


def join_backward(dtype, out_bordered, d1, d2, g, stride=1):
    """g = (d1 + d2) * [out > 0] between linked stacks (y2_join_backward); d2 fp32 or of the arithmetic type.
    stride 2: the unit above is a stride-2 unit, d2 lives on ITS output grid (y2_join_backward_s2)"""
    lib = _lib.load()
    dt = _lib.DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
    n, h, w, c = out_bordered.shape
    fn = lib.y2_join_backward if stride == 1 else lib.y2_join_backward_s2
    check(fn(dt, C.c_void_p(out_bordered.cell0), C.c_void_p(d1.data_ptr()), C.c_void_p(d2.data_ptr()),
             int(d2.dtype == torch.float32), C.c_void_p(g.data_ptr()), n, h, w, c, _stream()))
    return g


def subsample_bordered(dtype, src, dst):
    """resnet_utils.subsample(x, 2) between two Bordered tensors of the arithmetic type (y2_subsample_bordered)"""
    lib = _lib.load()
    dt = _lib.DTYPES[dtype] if isinstance(dtype, str) else int(dtype)
    n, h, w, c = src.shape
    assert tuple(dst.shape) == (n, h // 2, w // 2, c)
    check(lib.y2_subsample_bordered(dt, C.c_void_p(src.cell0), C.c_void_p(dst.cell0), n, h, w, c, _stream()))
    return dst


# ---------------------------------------------------------------------------
# flat-buffer optimizers
# ---------------------------------------------------------------------------
class LossScaler:
    """Dynamic loss scale for the half-precision modes (the fp32 reference has no counterpart).

    The guarded optimizer kernels skip a step whose gradient buffer holds an inf / NaN on the device, without a
    host synchronisation; this object reads the control words ONE STEP LATE (asynchronous copy into pinned
    memory) and halves grad_scale after an overflow, doubling it again after `growth_interval` clean steps up
    to the initial scale's ceiling.  ctrl words: found_inf, step, skipped, ticket, lr_t."""

    def __init__(self, net, growth_interval=2000, max_scale=65536.0, min_scale=1.0):
        self.net = net.scale_owner
        self.nets = [net]
        self.ctrl = torch.zeros(8, dtype=torch.int32, device=net.device)
        self._host = torch.zeros(8, dtype=torch.int32).pin_memory()
        self._event = None
        self.growth_interval, self.max_scale, self.min_scale = growth_interval, max_scale, min_scale
        self.enabled = net.dtype in _lib.LOSS_SCALED
        self._clean = 0
        self.overflows = 0

    @property
    def scale(self):
        return self.net.grad_scale

    def _apply(self, scale):
        seen = set()
        for n in [self.net] + self.nets:
            if id(n) not in seen:
                seen.add(id(n))
                n.set_grad_scale(scale)

    def attach(self, net):
        """another context on the same flat buffers (multi-scale): keep its scale in step"""
        if all(n is not net for n in self.nets):
            self.nets.append(net)
            net.set_grad_scale(self.scale)

    def scan(self, net, full=False, more=False):
        """set ctrl.found_inf from net's gradient buffer: sentinel ranges (default) or every element;
        more: OR into the flag another stack's scan of this step left (composed graphs: one all-or-nothing step)"""
        if full:
            check(net.lib.y2_grad_check_full(_ptr(net.grads), net.n_params, _ptr(self.ctrl), _stream()))
        elif more:
            check(net.lib.y2_grad_check_more(net.h, _ptr(self.ctrl), _stream()))
        else:
            check(net.lib.y2_grad_check(net.h, _ptr(self.ctrl), _stream()))

    def after_step(self):
        """call right after the guarded optimizer launch of a step"""
        if self._event is not None:          # the copy issued after the PREVIOUS step has long finished
            self._event.synchronize()
            if int(self._host[0]) != 0:
                self.overflows += 1
                self._clean = 0
                if self.enabled:
                    self._apply(max(self.scale * 0.5, self.min_scale))
            else:
                self._clean += 1
                if self.enabled and self._clean >= self.growth_interval and self.scale < self.max_scale:
                    self._clean = 0
                    self._apply(min(self.scale * 2.0, self.max_scale))
        self._host.copy_(self.ctrl, non_blocking=True)
        self._event = torch.cuda.Event()
        self._event.record()

    def state(self):
        """(found_inf, device step counter, skipped steps) -- synchronises"""
        c = self.ctrl.cpu().numpy()
        return int(c[0]), int(c[1]), int(c[2])


class _FlatOptimizer:
    """What the optimizers over a Network's flat buffers share: the guard (default: the loss-scaled modes) with its
    LossScaler, the bracket of a step (scan before, after_step after), backward_step's fallback and the tf.train.Saver
    slots.  A subclass names its slot tensors in SLOTS (created zeroed, exported and loaded by name), says with COUNTS
    whether it keeps a step counter `t`, and keeps its own step() and library calls."""
    SLOTS = ()
    COUNTS = True

    def __init__(self, net, guard, fused_pack):
        self.net = net
        self.fused_pack = bool(fused_pack)
        for k in self.SLOTS:
            setattr(self, k, torch.zeros_like(net.params))
        if self.COUNTS:
            self.t = 0
        self.guard = (net.dtype in _lib.LOSS_SCALED) if guard is None else bool(guard)
        self.scaler = LossScaler(net) if self.guard else None

    def _ctrl(self):
        return _ptr(self.scaler.ctrl) if self.guard else C.c_void_p(0)

    def _scan(self, full_check, joint=None):
        """before the launch of a step: the gradient scan (in a joint group the caller has scanned every stack into
        the shared flag) -> the ctrl pointer"""
        if self.guard and joint is None:
            self.scaler.scan(self.net, full_check)
        return self._ctrl()

    def _after(self, owner=True):
        """after the launch: once per step and shared scaler, by the call that owns the step"""
        if self.guard and owner:
            self.scaler.after_step()

    _train_op = None     # (dout, ctrl, grad_mult): backward + step + re-pack in one library call, where the solver has one

    def backward_step(self, dout, grad_mult=1.0):
        """train_op in one library call: net.backward(dout) + the (guarded) step + filter re-pack, with the update
        of the layers above the first one overlapped with the first layer's gradient kernel (single-process
        training; the data-parallel trainers reduce between backward() and step()).  Without the packed step, or
        for a solver that has no overlapped train op (DarknetSGD): net.backward(dout), then the step."""
        n = self.net
        if self._train_op is None or not (self.fused_pack and n.training) or os.environ.get("Y2_NO_FUSED_TRAIN_OP"):
            n.backward(dout)
            return self.step(grad_mult)
        if self.COUNTS:
            self.t += 1
        self._train_op(dout.contiguous(), self._ctrl(), grad_mult)
        self._after()

    # ---- tf.train.Saver slots (a resumed run must not restart Adam at t = 0)
    def export_state(self):
        st = {k: getattr(self, k).detach().cpu().numpy().copy() for k in self.SLOTS}
        if self.COUNTS:
            # the device counter is authoritative under a guard; `t` is its host mirror
            st["t"] = int(self.scaler.state()[1] if self.guard else self.t)
        return st

    def load_state(self, st):
        for k in self.SLOTS:
            slot = getattr(self, k)
            slot.copy_(torch.as_tensor(np.asarray(st[k], np.float32)).to(slot.device))
        if self.COUNTS:
            self.t = int(st["t"])
            if self.guard:
                c = self.scaler.ctrl.cpu()
                c[1] = self.t
                self.scaler.ctrl.copy_(c)


class AdamOptimizer(_FlatOptimizer):
    """tf.train.AdamOptimizer defaults (src/pascal/pascal_train_darknet.py:51).
    guard=True (default for the f16 mode): the overflow-safe kernels + LossScaler; the step counter then lives
    on the device (`t` mirrors it assuming no skipped step; `scaler.state()` is authoritative)."""
    SLOTS = ("m", "v")

    def __init__(self, net, learning_rate=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8, guard=None, fused_pack=True):
        _FlatOptimizer.__init__(self, net, guard, fused_pack)
        self.lr, self.b1, self.b2, self.eps = learning_rate, beta1, beta2, epsilon

    def step(self, grad_mult=1.0, full_check=False, joint=None):
        """full_check: scan every gradient element instead of the sentinel ranges (a gradient buffer that was
        not produced by this context's backward pass).
        joint: None, or this optimizer's place in a group that shares ONE LossScaler over a composed graph
        ("first": the caller has scanned every stack into the shared flag -- advance the step counter once;
        "next": use the counter / lr_t the first stack's call advanced)."""
        self.t += 1
        n = self.net
        ctrl = self._scan(full_check, joint)
        owner = joint is None or joint == "first"
        if joint is not None:
            assert self.guard and self.fused_pack and n.training
        if self.fused_pack and n.training:
            # update + filter re-pack in one pass over the parameters (the context's packed copies stay current)
            check(n.lib.y2_adam_step_packed(n.h, _ptr(self.m), _ptr(self.v), ctrl, self.t if owner else -1, self.lr,
                                            self.b1, self.b2, self.eps, grad_mult, _stream()))
        elif self.guard:
            check(n.lib.y2_adam_step_guarded(_ptr(n.params), _ptr(self.m), _ptr(self.v), _ptr(n.grads), n.n_params,
                                             ctrl, self.lr, self.b1, self.b2, self.eps, grad_mult, _stream()))
            n.params_changed()
        else:
            check(n.lib.y2_adam_step(_ptr(n.params), _ptr(self.m), _ptr(self.v), _ptr(n.grads), n.n_params, self.t,
                                     self.lr, self.b1, self.b2, self.eps, grad_mult, _stream()))
            n.params_changed()
        self._after(owner)

    def _train_op(self, dout, ctrl, grad_mult):
        n = self.net
        check(n.lib.y2_backward_adam(n.h, _ptr(dout), _ptr(self.m), _ptr(self.v), ctrl, self.t, self.lr, self.b1,
                                     self.b2, self.eps, grad_mult, _stream()))


class MomentumOptimizer(_FlatOptimizer):
    """tf.train.MomentumOptimizer(0.001, 0.9) (src/imagenet/imagenet_train_darknet.py:58)."""
    SLOTS = ("accum",)
    COUNTS = False

    def __init__(self, net, learning_rate=1e-3, momentum=0.9, guard=None, fused_pack=True):
        _FlatOptimizer.__init__(self, net, guard, fused_pack)
        self.lr, self.mom = learning_rate, momentum

    def step(self, grad_mult=1.0, full_check=False):
        n = self.net
        ctrl = self._scan(full_check)
        if self.fused_pack and n.training:
            check(n.lib.y2_momentum_step_packed(n.h, _ptr(self.accum), ctrl, self.lr, self.mom, grad_mult, _stream()))
        elif self.guard:
            check(n.lib.y2_momentum_step_guarded(_ptr(n.params), _ptr(self.accum), _ptr(n.grads), n.n_params,
                                                 ctrl, self.lr, self.mom, grad_mult, _stream()))
            n.params_changed()
        else:
            check(n.lib.y2_momentum_step(_ptr(n.params), _ptr(self.accum), _ptr(n.grads), n.n_params, self.lr,
                                         self.mom, grad_mult, _stream()))
            n.params_changed()
        self._after()

    def _train_op(self, dout, ctrl, grad_mult):
        n = self.net
        check(n.lib.y2_backward_momentum(n.h, _ptr(dout), _ptr(self.accum), ctrl, self.lr, self.mom, grad_mult,
                                         _stream()))


class DarknetSGD(_FlatOptimizer):
    """Darknet's solver for the YOLOv2 anchor model (not in the reference; specification utils/solver.py): momentum
    SGD with weight decay on the convolution filters only and a rate schedule (burn-in, then constant / steps / poly).
    `solver`: a utils.solver.Solver.  The shape of AdamOptimizer: guarded in the loss-scaled modes, where the step
    counter AND the schedule live on the device -- a skipped step moves neither (`t` mirrors the counter assuming no
    skipped step; `scaler.state()` is authoritative, word 4 of `scaler.ctrl` holds the rate last applied)."""
    SLOTS = ("accum",)

    def __init__(self, net, solver, guard=None, fused_pack=True):
        _FlatOptimizer.__init__(self, net, guard, fused_pack)
        self.solver = solver
        self._record = _lib.sgd_solver(solver)

    def step(self, grad_mult=1.0, full_check=False, joint=None):
        """full_check / joint: see AdamOptimizer.step"""
        self.t += 1
        n = self.net
        if not n.training:
            raise ValueError("DarknetSGD steps a context bound for training")
        ctrl = self._scan(full_check, joint)
        if joint is not None:
            assert self.guard and self.fused_pack
        fn = n.lib.y2_sgd_step_packed if self.fused_pack else n.lib.y2_sgd_step
        check(fn(n.h, _ptr(self.accum), ctrl, -1 if joint == "next" else self.t, C.byref(self._record), grad_mult,
                 _stream()))
        if not self.fused_pack:
            n.params_changed()
        self._after(joint != "next")


# ---------------------------------------------------------------------------
# loss / decode ops on device tensors
# ---------------------------------------------------------------------------
LAMBDA_COORD = 5.0   # src/config.py:44
LAMBDA_NOOBJ = 0.5   # src/config.py:45


def yolo_loss(net, labels, num_class, batch_size, image_size, S, B, need_grad=True,
              lambda_coord=LAMBDA_COORD, lambda_noobj=LAMBDA_NOOBJ):
    """get_loss (src/yolo2_nets/net_utils.py:263-372) forward (+ d loss / d net).
    Returns (loss[5] = class, object, noobject, coord, total; ious; object_mask; dnet or None)."""
    lib = _lib.load()
    assert net.is_cuda and labels.is_cuda
    net = net.contiguous().float()
    labels = labels.contiguous().float()
    assert net.numel() == batch_size * S * S * (num_class + 5 * B), "net shape does not match batch_size/S/B"
    assert labels.numel() == batch_size * S * S * (5 + num_class)
    dev = net.device
    loss = torch.empty(5, dtype=torch.float32, device=dev)
    ious = torch.empty((batch_size, S, S, B), dtype=torch.float32, device=dev)
    mask = torch.empty((batch_size, S, S, B), dtype=torch.float32, device=dev)
    dnet = torch.empty((batch_size, S, S, num_class + 5 * B), dtype=torch.float32, device=dev) if need_grad else None
    ws = torch.empty(lib.y2_yolo_loss_workspace_bytes(batch_size, S), dtype=torch.uint8, device=dev)
    check(lib.y2_yolo_loss(_ptr(net), _ptr(labels), num_class, batch_size, float(image_size), S, B,
                           lambda_coord, lambda_noobj, _ptr(loss), _ptr(ious), _ptr(mask), _ptr(dnet), _ptr(ws),
                           _stream()))
    return loss, ious, mask, dnet


def get_iou(boxes1, boxes2):
    """src/yolo2_nets/net_utils.py:222-260 on [..., 4] device tensors."""
    lib = _lib.load()
    b1 = boxes1.contiguous().float()
    b2 = boxes2.contiguous().float()
    assert b1.shape == b2.shape and b1.shape[-1] == 4
    out = torch.empty(b1.shape[:-1], dtype=torch.float32, device=b1.device)
    check(lib.y2_get_iou(_ptr(b1), _ptr(b2), _ptr(out), out.numel(), _stream()))
    return out


def decode_detections(predict, S, B, num_class, im_w, im_h, object_thresh=0.5):
    """Arithmetic of show_yolo_detection (src/yolo2_nets/net_utils.py:393-421).
    Returns the reference's tuples (ulx, uly, w, h, cls, conf, c, r, i) in its loop order."""
    lib = _lib.load()
    p = predict.contiguous().float().view(-1)
    assert p.numel() == S * S * (num_class + 5 * B)
    det = torch.empty((S * S * B, 8), dtype=torch.int32, device=p.device)
    conf = torch.empty(S * S * B, dtype=torch.float32, device=p.device)
    check(lib.y2_decode_detections(_ptr(p), S, B, num_class, im_w, im_h, float(object_thresh), _ptr(det),
                                   _ptr(conf), _stream()))
    det = det.cpu().numpy()
    conf = conf.cpu().numpy()
    out = []
    for i in range(S * S * B):
        if det[i, 0]:
            out.append((int(det[i, 1]), int(det[i, 2]), int(det[i, 3]), int(det[i, 4]), int(det[i, 5]),
                        float(conf[i]), int(det[i, 6]), int(det[i, 7]), i % B))
    return out


# ---- YOLOv2 pieces beyond the reference (SURVEY §8 a-x1/a-x2; specification: oracle/ext_ref.py) ----------
def max_pool_2x2(x):
    """tf.nn.max_pool(x, 2, 2, 'SAME') on [N,H,W,C] fp32 (darknet.py:24-25)"""
    lib = _lib.load()
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4
    n, h, w, c = x.shape
    y = torch.empty((n, (h + 1) // 2, (w + 1) // 2, c), dtype=torch.float32, device=x.device)
    check(lib.y2_maxpool2x2(_ptr(x), _ptr(y), n, h, w, c, _stream()))
    return y


def max_pool_2x2_backward(x, dy):
    lib = _lib.load()
    n, h, w, c = x.shape
    assert x.is_contiguous() and dy.is_contiguous() and tuple(dy.shape) == (n, (h + 1) // 2, (w + 1) // 2, c)
    dx = torch.empty_like(x)
    check(lib.y2_maxpool2x2_backward(_ptr(x), _ptr(dy), _ptr(dx), n, h, w, c, _stream()))
    return dx


def max_pool_2x2_s1(x):
    """Darknet's `[maxpool] size=2 stride=1` on [N,H,W,C] fp32 -> [N,H,W,C]: the window anchored top-left, clipped at the
    bottom and right edges (utils/darknet_maxpool.maxpool_s1, bit-equal)"""
    lib = _lib.load()
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError("max_pool_2x2_s1: x %s is no non-empty [N,H,W,C]" % (tuple(x.shape),))
    n, h, w, c = x.shape
    y = torch.empty((n, h, w, c), dtype=torch.float32, device=x.device)
    check(lib.y2_maxpool2x2s1(_ptr(x), _ptr(y), n, h, w, c, _stream()))
    return y


def max_pool_2x2_s1_backward(x, dy):
    """the gradient of max_pool_2x2_s1 (utils/darknet_maxpool.maxpool_s1_backward, bit-equal): every dx element written once"""
    lib = _lib.load()
    assert x.is_cuda and dy.is_cuda and x.dtype == dy.dtype == torch.float32 and x.is_contiguous() and dy.is_contiguous()
    if x.dim() != 4 or x.numel() == 0 or dy.shape != x.shape:
        raise ValueError("max_pool_2x2_s1_backward: x %s must be a non-empty [N,H,W,C] and dy %s of its shape" %
                         (tuple(x.shape), tuple(dy.shape)))
    n, h, w, c = x.shape
    dx = torch.empty_like(x)
    check(lib.y2_maxpool2x2s1_backward(_ptr(x), _ptr(dy), _ptr(dx), n, h, w, c, _stream()))
    return dx


def reorg(x, stride=2, inverse=False):
    """space-to-depth [N,H,W,C] -> [N,H/s,W/s,s*s*C]; inverse=True: the gradient (depth-to-space)"""
    lib = _lib.load()
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4
    s = int(stride)
    if not inverse:
        n, h, w, c = x.shape
        y = torch.empty((n, h // s, w // s, s * s * c), dtype=torch.float32, device=x.device)
        check(lib.y2_reorg(_ptr(x), _ptr(y), n, h, w, c, s, 1, _stream()))
    else:
        n, ho, wo, cc = x.shape
        c = cc // (s * s)
        y = torch.empty((n, ho * s, wo * s, c), dtype=torch.float32, device=x.device)
        check(lib.y2_reorg(_ptr(x), _ptr(y), n, ho * s, wo * s, c, s, 0, _stream()))
    return y


def passthrough_concat(fine, coarse):
    """concat(reorg2(fine [N,2H,2W,Cf]), coarse [N,H,W,Cc]) -> [N,H,W,4*Cf+Cc]"""
    lib = _lib.load()
    n, h, w, cc = coarse.shape
    cf = fine.shape[3]
    assert tuple(fine.shape[:3]) == (n, 2 * h, 2 * w) and fine.is_contiguous() and coarse.is_contiguous()
    out = torch.empty((n, h, w, 4 * cf + cc), dtype=torch.float32, device=coarse.device)
    check(lib.y2_passthrough_concat(_ptr(fine), _ptr(coarse), _ptr(out), n, h, w, cf, cc, _stream()))
    return out


def passthrough_concat_darknet(fine, coarse, out=None):
    """Darknet's passthrough (utils/darknet_reorg.passthrough_concat_darknet): concat(Darknet's reorg of fine
    [N,2H,2W,Cf], coarse [N,H,W,Cc]) -> [N,H,W,4*Cf+Cc], one launch (gradient: passthrough_concat_darknet_backward)"""
    lib = _lib.load()
    n, h, w, cc = coarse.shape
    cf = fine.shape[3]
    assert fine.is_cuda and coarse.is_cuda and fine.dtype == coarse.dtype == torch.float32
    assert tuple(fine.shape[:3]) == (n, 2 * h, 2 * w) and fine.is_contiguous() and coarse.is_contiguous()
    if out is None:
        out = torch.empty((n, h, w, 4 * cf + cc), dtype=torch.float32, device=coarse.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n * h * w * (4 * cf + cc)
    check(lib.y2_passthrough_concat_darknet(_ptr(fine), _ptr(coarse), _ptr(out), n, h, w, cf, cc, _stream()))
    return out


def u8_to_darknet_input(images_u8, out=None):
    """uint8 BGR pixels [..., 3] (DeviceVOC.eval_batch, DeviceImages.batch) -> float32 RGB in [0, 1] of the same shape,
    Darknet's network input: out[..., c] = float32(images_u8[..., 2 - c]) / 255"""
    lib = _lib.load()
    assert images_u8.is_cuda and images_u8.dtype == torch.uint8 and images_u8.is_contiguous() and images_u8.shape[-1] == 3
    if out is None:
        out = torch.empty(images_u8.shape, dtype=torch.float32, device=images_u8.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == images_u8.numel()
    check(lib.y2_u8_bgr_to_f32_rgb(_ptr(images_u8), _ptr(out), images_u8.numel() // 3, _stream()))
    return out


def passthrough_concat_backward(dout, cf):
    lib = _lib.load()
    n, h, w, ct = dout.shape
    cc = ct - 4 * cf
    assert dout.is_contiguous()
    dfine = torch.empty((n, 2 * h, 2 * w, cf), dtype=torch.float32, device=dout.device)
    dcoarse = torch.empty((n, h, w, cc), dtype=torch.float32, device=dout.device)
    check(lib.y2_passthrough_concat_backward(_ptr(dout), _ptr(dfine), _ptr(dcoarse), n, h, w, cf, cc, _stream()))
    return dfine, dcoarse


def passthrough_concat_darknet_backward(dout, cf, dfine_out=None, dcoarse_out=None):
    """the gradient of passthrough_concat_darknet (utils/darknet_reorg.passthrough_concat_darknet_backward): dout
    [N,H,W,4*cf+Cc] -> (dfine [N,2H,2W,cf], dcoarse [N,H,W,Cc]), one launch that writes every element of both once"""
    lib = _lib.load()
    assert dout.is_cuda and dout.dtype == torch.float32 and dout.is_contiguous() and dout.dim() == 4
    n, h, w, ct = dout.shape
    cf = int(cf)
    cc = ct - 4 * cf
    if dfine_out is None:
        dfine_out = torch.empty((n, 2 * h, 2 * w, cf), dtype=torch.float32, device=dout.device)
    if dcoarse_out is None:
        dcoarse_out = torch.empty((n, h, w, max(cc, 0)), dtype=torch.float32, device=dout.device)
    for t, count in ((dfine_out, n * 4 * h * w * cf), (dcoarse_out, n * h * w * cc)):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == max(count, 0)
    check(lib.y2_passthrough_concat_darknet_backward(_ptr(dout), _ptr(dfine_out), _ptr(dcoarse_out), n, h, w, cf, cc,
                                                     _stream()))
    return dfine_out, dcoarse_out


def zero_(x):
    """x[:] = 0 on a contiguous fp32 device tensor or view (gradient masks of a trainer)"""
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    check(_lib.load().y2_zero(_ptr(x), x.numel(), _stream()))
    return x


def add_relu(a, b):
    """relu(a + b): the join of a ResNet bottleneck unit (slim_dir/nets/resnet_v1.py:112)"""
    lib = _lib.load()
    assert a.is_cuda and a.dtype == b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous() and a.shape == b.shape
    out = torch.empty_like(a)
    check(lib.y2_add_relu(_ptr(a), _ptr(b), _ptr(out), a.numel(), _stream()))
    return out


def add_relu_backward(dout, out, dout2=None):
    """(dout + dout2) * [out > 0]: the gradient of both addends of add_relu (dout2: a second part of the incoming gradient)"""
    lib = _lib.load()
    assert dout.is_cuda and dout.dtype == out.dtype == torch.float32 and dout.is_contiguous() and out.is_contiguous()
    assert dout2 is None or (dout2.is_contiguous() and dout2.dtype == torch.float32 and dout2.shape == dout.shape)
    g = torch.empty_like(dout)
    check(lib.y2_add_relu_backward(_ptr(dout), _ptr(dout2), _ptr(out), _ptr(g), dout.numel(), _stream()))
    return g


def accumulate(dst, src):
    """dst += src (fp32 device tensors of equal size)"""
    lib = _lib.load()
    assert dst.is_cuda and dst.dtype == torch.float32 and dst.is_contiguous() and src.is_contiguous()
    assert dst.numel() == src.numel() and src.dtype == torch.float32
    check(lib.y2_accumulate(_ptr(dst), _ptr(src), dst.numel(), _stream()))
    return dst


def class_argmax(scores):
    """scores [..., C] -> (best [...], class index [...] int32); ties: the smallest index"""
    lib = _lib.load()
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.is_contiguous()
    c = scores.shape[-1]
    rows = scores.numel() // c
    best = torch.empty(scores.shape[:-1], dtype=torch.float32, device=scores.device)
    cls = torch.empty(scores.shape[:-1], dtype=torch.int32, device=scores.device)
    check(lib.y2_class_argmax(_ptr(scores), _ptr(best), _ptr(cls), rows, c, _stream()))
    return best, cls


def decode_anchors(net, anchors):
    """net [N,S,S,B,5+C], anchors [B,2] -> boxes [N,S*S*B,4], scores [N,S*S*B,C]"""
    lib = _lib.load()
    n, s, _, b, d = net.shape
    c = d - 5
    assert net.is_cuda and net.dtype == torch.float32 and net.is_contiguous()
    an = _upload_anchors(anchors, net.device)
    boxes = torch.empty((n, s * s * b, 4), dtype=torch.float32, device=net.device)
    scores = torch.empty((n, s * s * b, c), dtype=torch.float32, device=net.device)
    check(lib.y2_decode_anchors(_ptr(net), _ptr(an), _ptr(boxes), _ptr(scores), n, s, b, c, _stream()))
    return boxes, scores


def yolov2_loss(net, labels, anchors, image_size, need_grad=True, scales=None):
    """anchor-box loss of the YOLOv2 head (oracle/ext_ref.py yolov2_loss): net [N,S,S,B,5+C], labels [N,S,S,5+C]
    -> (loss[5] = coord, object, noobject, class, total; dnet or None)"""
    lib = _lib.load()
    assert net.is_cuda and net.dtype == torch.float32 and net.is_contiguous() and net.dim() == 5
    n, s, _, b, d = net.shape
    labels = labels.contiguous().float()
    assert tuple(labels.shape) == (n, s, s, d), labels.shape
    an = _upload_anchors(anchors, net.device)
    sc = None
    if scales is not None:
        sc = torch.as_tensor(np.asarray([scales[k] for k in ("coord_scale", "object_scale", "noobject_scale",
                                                              "class_scale", "thresh")], np.float32)).to(net.device)
    loss = torch.empty(5, dtype=torch.float32, device=net.device)
    dnet = torch.empty_like(net) if need_grad else None
    ws = torch.empty(lib.y2_yolov2_loss_workspace_bytes(n), dtype=torch.uint8, device=net.device)
    check(lib.y2_yolov2_loss(_ptr(net), _ptr(labels), _ptr(an), n, s, b, d - 5, float(image_size), _ptr(sc), _ptr(loss),
                             _ptr(dnet), _ptr(ws), _stream()))
    return loss, dnet


BOX_LOSS_SCALES = ("coord_scale", "object_scale", "noobject_scale", "class_scale", "thresh", "area_weight", "prior_scale")
_BOX_LOSS_DEFAULTS = (1.0, 5.0, 1.0, 1.0, 0.6, 0.0, 0.0)


def yolov2_loss_boxes(net, truth, ntruth, anchors, image_size, need_grad=True, scales=None):
    """anchor-box loss of the YOLOv2 head on box lists (utils/region_loss.py yolov2_loss_boxes): net [N,S,S,B,5+C], truth
    [N,T,5] float32 = cx, cy, w, h in pixels and the class index, ntruth [N] int32 (img_dataset/augment.encode_box_list)
    -> (loss[5] = coord, object, noobject, class, total; dnet or None).  scales: a dict with any of BOX_LOSS_SCALES
    (missing keys take the defaults 1, 5, 1, 1, 0.6, no area weight, no prior)."""
    lib = _lib.load()
    assert net.is_cuda and net.dtype == torch.float32 and net.is_contiguous() and net.dim() == 5
    n, s, _, b, d = net.shape
    assert truth.is_cuda and truth.dtype == torch.float32 and truth.is_contiguous(), (truth.dtype, truth.device)
    assert truth.dim() == 3 and truth.shape[0] == n and truth.shape[2] == 5, truth.shape
    assert ntruth.is_cuda and ntruth.dtype == torch.int32 and ntruth.is_contiguous() and tuple(ntruth.shape) == (n,)
    an = _upload_anchors(anchors, net.device)
    assert tuple(an.shape) == (b, 2), an.shape
    sc = None
    if scales is not None:
        unknown = set(scales) - set(BOX_LOSS_SCALES)
        if unknown:
            raise ValueError("unknown loss scales %s" % sorted(unknown))
        sc = (C.c_float * 7)(*[float(scales.get(k, v)) for k, v in zip(BOX_LOSS_SCALES, _BOX_LOSS_DEFAULTS)])   # host memory
    loss = torch.empty(5, dtype=torch.float32, device=net.device)
    dnet = torch.empty_like(net) if need_grad else None
    ws = torch.empty(lib.y2_yolov2_loss_boxes_workspace_bytes(n, s, b), dtype=torch.uint8, device=net.device)
    check(lib.y2_yolov2_loss_boxes(_ptr(net), _ptr(truth), _ptr(ntruth), _ptr(an), n, s, b, d - 5, int(truth.shape[1]),
                                   float(image_size), sc, _ptr(loss), _ptr(dnet), _ptr(ws), _stream()))
    return loss, dnet


def yolov2_region_stats(net, truth, ntruth, anchors, image_size, out=None):
    """the numbers of Darknet's region-layer log line (utils/region_loss.py region_stats_boxes) from the tensors
    yolov2_loss_boxes reads: net [N,S,S,B,5+C], truth [N,T,5], ntruth [N], anchors [B,2] (anything numpy reads, or a
    float32 device tensor) -> stats float32 [6] on the device (in `out` if
    given) = mean IoU, mean class probability, mean objectness at the truths, mean objectness over every slot, recall at
    IoU 0.5, truth count.  No host synchronisation; the result does not vary from run to run"""
    lib = _lib.load()
    assert net.is_cuda and net.dtype == torch.float32 and net.is_contiguous() and net.dim() == 5
    n, s, _, b, d = net.shape
    assert truth.is_cuda and truth.dtype == torch.float32 and truth.is_contiguous(), (truth.dtype, truth.device)
    assert truth.dim() == 3 and truth.shape[0] == n and truth.shape[2] == 5, truth.shape
    assert ntruth.is_cuda and ntruth.dtype == torch.int32 and ntruth.is_contiguous() and tuple(ntruth.shape) == (n,)
    an = _anchors(anchors, b, net.device)                 # a device tensor is taken as it is: no copy per call
    if out is None:
        out = torch.empty(6, dtype=torch.float32, device=net.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == 6, (out.dtype, out.shape)
    ws = torch.empty(lib.y2_yolov2_region_stats_workspace_bytes(n), dtype=torch.uint8, device=net.device)
    check(lib.y2_yolov2_region_stats(_ptr(net), _ptr(truth), _ptr(ntruth), _ptr(an), n, s, b, d - 5, int(truth.shape[1]),
                                     float(image_size), _ptr(out), _ptr(ws), _stream()))
    return out


class WordTreeTables:
    """the word tree of a region layer on the device (utils/word_tree.py): the record's packed int32 tables, uploaded
    once, with the counts the entries take next to them.  `tree`: a utils.word_tree.WordTree record"""

    def __init__(self, tree, device="cuda:0"):
        from .utils import word_tree
        self.tree, self.n, self.groups, self.max_depth = tree, int(tree.n), word_tree.groups(tree), int(tree.max_depth)
        self.tables = torch.as_tensor(word_tree.pack(tree)).to(device).contiguous()


def _tree(tree, c, device):
    """tree: WordTreeTables on the device of the call, of exactly c nodes"""
    assert isinstance(tree, WordTreeTables) and tree.tables.device == device, "tree"
    if tree.n != c:
        raise ValueError("the word tree holds %d nodes, the head %d classes" % (tree.n, c))
    return tree


def yolov2_loss_boxes_tree(net, truth, ntruth, anchors, image_size, tree, need_grad=True, scales=None):
    """yolov2_loss_boxes with the class term of the word tree (utils/word_tree.py yolov2_loss_boxes_tree): the same
    tensors, scales and results; tree: WordTreeTables of C nodes; a truth's class is a node index, any node"""
    lib = _lib.load()
    assert net.is_cuda and net.dtype == torch.float32 and net.is_contiguous() and net.dim() == 5
    n, s, _, b, d = net.shape
    tree = _tree(tree, d - 5, net.device)
    assert truth.is_cuda and truth.dtype == torch.float32 and truth.is_contiguous(), (truth.dtype, truth.device)
    assert truth.dim() == 3 and truth.shape[0] == n and truth.shape[2] == 5, truth.shape
    assert ntruth.is_cuda and ntruth.dtype == torch.int32 and ntruth.is_contiguous() and tuple(ntruth.shape) == (n,)
    an = _anchors(anchors, b, net.device)
    sc = None
    if scales is not None:
        unknown = set(scales) - set(BOX_LOSS_SCALES)
        if unknown:
            raise ValueError("unknown loss scales %s" % sorted(unknown))
        sc = (C.c_float * 7)(*[float(scales.get(k, v)) for k, v in zip(BOX_LOSS_SCALES, _BOX_LOSS_DEFAULTS)])   # host memory
    loss = torch.empty(5, dtype=torch.float32, device=net.device)
    dnet = torch.empty_like(net) if need_grad else None
    ws = torch.empty(lib.y2_yolov2_loss_boxes_tree_workspace_bytes(n, s, b), dtype=torch.uint8, device=net.device)
    check(lib.y2_yolov2_loss_boxes_tree(_ptr(net), _ptr(truth), _ptr(ntruth), _ptr(an), _ptr(tree.tables), n, s, b, d - 5,
                                        tree.groups, tree.max_depth, int(truth.shape[1]), float(image_size), sc,
                                        _ptr(loss), _ptr(dnet), _ptr(ws), _stream()))
    return loss, dnet


def yolov2_region_stats_tree(net, truth, ntruth, anchors, image_size, tree, out=None):
    """yolov2_region_stats with the class statistic of the word tree (utils/word_tree.py region_stats_boxes_tree): the mean
    of abs[class] over the truths; tree: WordTreeTables of C nodes"""
    lib = _lib.load()
    assert net.is_cuda and net.dtype == torch.float32 and net.is_contiguous() and net.dim() == 5
    n, s, _, b, d = net.shape
    tree = _tree(tree, d - 5, net.device)
    assert truth.is_cuda and truth.dtype == torch.float32 and truth.is_contiguous(), (truth.dtype, truth.device)
    assert truth.dim() == 3 and truth.shape[0] == n and truth.shape[2] == 5, truth.shape
    assert ntruth.is_cuda and ntruth.dtype == torch.int32 and ntruth.is_contiguous() and tuple(ntruth.shape) == (n,)
    an = _anchors(anchors, b, net.device)
    out = _own(out, (6,), torch.float32, net.device, numel=6)
    ws = torch.empty(lib.y2_yolov2_region_stats_workspace_bytes(n), dtype=torch.uint8, device=net.device)
    check(lib.y2_yolov2_region_stats_tree(_ptr(net), _ptr(truth), _ptr(ntruth), _ptr(an), _ptr(tree.tables), n, s, b, d - 5,
                                          tree.groups, tree.max_depth, int(truth.shape[1]), float(image_size), _ptr(out),
                                          _ptr(ws), _stream()))
    return out


def word_tree_head(net, tree, tree_thresh=0.5, out=None, want_top=False):
    """the detection head of a word tree (utils/word_tree.py word_tree_head): net [..., 5+C] fp32 -> the same shape with
    elements 0..4 copied and the class logits 0 at the predicted node, -inf elsewhere, which every detect entry reads as
    score sig(to) at that node (in `out` if given; out = net rewrites in place).  want_top: -> (out, top int32 [rows],
    prob [rows] = abs[top]).  tree: WordTreeTables of C nodes"""
    lib = _lib.load()
    _dev(net, torch.float32, "net")
    d = int(net.shape[-1])
    tree = _tree(tree, d - 5, net.device)
    rows = net.numel() // d
    out = _own(out, net.shape, torch.float32, net.device, numel=net.numel())
    top = torch.empty(rows, dtype=torch.int32, device=net.device) if want_top else None
    prob = torch.empty(rows, dtype=torch.float32, device=net.device) if want_top else None
    check(lib.y2_word_tree_head(_ptr(net), _ptr(tree.tables), rows, d - 5, tree.groups, tree.max_depth, float(tree_thresh),
                                _ptr(out), _ptr(top), _ptr(prob), _stream()))
    return (out, top, prob) if want_top else out


def word_tree_top(net, tree, tree_thresh=0.5, obj_thresh=None, out=None):
    """word_tree_head's walk without the rewrite: net [..., 5+C] fp32, read only -> (top int32 [rows], prob [rows] =
    abs[top]), bit for bit what word_tree_head(want_top=True) returns (in out = (top, prob) if given).  obj_thresh (None:
    every row is walked): a row whose objectness sig(to) is not > obj_thresh gets top -1, prob 0 and none of its class
    logits is read -- the rows detect_anchor_tree_batch drops at score_thresh = obj_thresh anyway.  One launch"""
    lib = _lib.load()
    _dev(net, torch.float32, "net")
    d = int(net.shape[-1])
    tree = _tree(tree, d - 5, net.device)
    rows = net.numel() // d
    top, prob = out if out is not None else (None, None)
    top = _own(top, (rows,), torch.int32, net.device, numel=rows)
    prob = _own(prob, (rows,), torch.float32, net.device, numel=rows)
    check(lib.y2_word_tree_top(_ptr(net), _ptr(tree.tables), rows, d - 5, tree.groups, tree.max_depth, float(tree_thresh),
                               -1.0 if obj_thresh is None else float(obj_thresh), _ptr(top), _ptr(prob), _stream()))
    return top, prob


WIDE_HEAD_DTYPES = ("f16", "fp8")    # the model modes a wide head runs behind: its one arithmetic is f16 x f16 -> fp32


class WideHead:
    """a 1x1 convolution wider than a stack's 2,048-column row (YOLO9000's last layer, 1024 -> 28,269), run behind the
    head stack by csrc/wide_head.hip: out[m][c] = b[c] + sum_k f16(x[m][k]) f16(W[k][c]), fp32 accumulation, and trained by
    csrc/wide_head_train.hip (backward; WideHeadSGD steps it).  Holds the fp32 filters [1][1][K][Cout] and bias (what
    export() returns and a `.weights` file takes back), the two packed f16 operand images the kernels read -- `packed`
    [Cp][Kp] for the forward pass, `packed2` [Kp2][Cp2] for the data gradient -- one output buffer per M and, once
    backward() has run, the gradients dW / db, one dx buffer per M and the workspace of the split reductions"""

    def __init__(self, K, Cout, device="cuda:0"):
        self.lib = _lib.load()
        self.K, self.Cout, self.device = int(K), int(Cout), torch.device(device)
        nbytes = self.lib.y2_wide_head_packed_bytes(self.K, self.Cout)
        if nbytes == 0:
            raise ValueError("WideHead: K = %d (a multiple of 32, at most 4096), Cout = %d (1..%d)" %
                             (self.K, self.Cout, 65536 * 16))
        self.W = torch.zeros((1, 1, self.K, self.Cout), dtype=torch.float32, device=self.device)
        self.b = torch.zeros(self.Cout, dtype=torch.float32, device=self.device)
        self.packed = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.packed2 = torch.empty(self.lib.y2_wide_head_packed2_bytes(self.K, self.Cout), dtype=torch.uint8,
                                   device=self.device)
        self.dW = self.db = None             # allocated by the first backward(): a detector's operator holds none
        self._out, self._dx, self._ws = {}, {}, None
        self._pack()

    def _pack(self):
        check(self.lib.y2_wide_head_pack(_ptr(self.W), self.K, self.Cout, _ptr(self.packed), self.packed.numel(), _stream()))
        check(self.lib.y2_wide_head_pack2(_ptr(self.W), self.K, self.Cout, _ptr(self.packed2), self.packed2.numel(),
                                          _stream()))

    def load(self, W, b):
        """W: anything numpy reads of K * Cout values in the order [K][Cout] (a 1x1 layer's [1][1][K][Cout]); b [Cout]"""
        W, b = np.asarray(W, np.float32), np.asarray(b, np.float32)
        if W.size != self.K * self.Cout or b.shape != (self.Cout,):
            raise ValueError("WideHead.load: W %s and b %s do not fit %d -> %d" % (W.shape, b.shape, self.K, self.Cout))
        self.W.copy_(torch.as_tensor(np.ascontiguousarray(W).reshape(1, 1, self.K, self.Cout)).to(self.device))
        self.b.copy_(torch.as_tensor(b).to(self.device))
        self._pack()

    def export(self):
        """-> {"W": [1][1][K][Cout], "b": [Cout]} as numpy arrays: the fp32 values load() was given"""
        return {"W": self.W.cpu().numpy().copy(), "b": self.b.cpu().numpy().copy()}

    def export_grads(self):
        """-> {"W": [1][1][K][Cout], "b": [Cout]}: the gradients the last backward() left"""
        if self.dW is None:
            raise ValueError("WideHead.export_grads: backward() has not run")
        return {"W": self.dW.cpu().numpy().copy(), "b": self.db.cpu().numpy().copy()}

    def forward(self, x, out=None):
        """x: fp32 [..., K] on the device, contiguous -> fp32 [M][Cout], M the product of the leading sizes (in `out`, a
        contiguous fp32 tensor of M * Cout elements, if given; else in this operator's buffer for that M)"""
        _dev(x, torch.float32, "x")
        assert x.shape[-1] == self.K, (tuple(x.shape), self.K)
        m = x.numel() // self.K
        if out is None:
            out = self._out.get(m)
            if out is None:
                out = self._out[m] = torch.empty((m, self.Cout), dtype=torch.float32, device=self.device)
        else:
            _own(out, None, torch.float32, self.device, numel=m * self.Cout)
        check(self.lib.y2_wide_head_forward(_ptr(x), _ptr(self.packed), _ptr(self.b), m, self.K, self.Cout, _ptr(out),
                                            _stream()))
        return out

    def backward(self, x, dy, grad_scale=1.0, want_dx=True, _split=(0, 0)):
        """x: fp32 [..., K], the input forward() was given; dy: fp32 of M * Cout elements, the gradient at its output,
        UNSCALED; grad_scale: the loss scale the operands are rounded under.  Fills self.dW [1][1][K][Cout] and self.db
        [Cout] (unscaled) and returns dx fp32 [M][K] in this operator's buffer for that M (None unless want_dx).
        _split: (dx, dW) split counts in place of the plan's, 0 the plan's (tests and measurements)"""
        _dev(x, torch.float32, "x")
        _dev(dy, torch.float32, "dy")
        assert x.shape[-1] == self.K, (tuple(x.shape), self.K)
        m = x.numel() // self.K
        assert dy.numel() == m * self.Cout, (tuple(dy.shape), m, self.Cout)
        lib, (sx, sw) = self.lib, _split
        if self.dW is None:
            self.dW, self.db = torch.empty_like(self.W), torch.empty_like(self.b)
        need = lib.y2_wide_head_backward_filter_workspace_bytes(m, self.K, self.Cout, sw)
        if want_dx:
            need = max(need, lib.y2_wide_head_backward_input_workspace_bytes(m, self.K, self.Cout, sx))
        if need and (self._ws is None or self._ws.numel() < need):
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        nws = self._ws.numel() if self._ws is not None else 0
        check(lib.y2_wide_head_backward_filter(_ptr(x), _ptr(dy), m, self.K, self.Cout, float(grad_scale), _ptr(self.dW),
                                               _ptr(self.db), _ptr(self._ws), nws, sw, _stream()))
        if not want_dx:
            return None
        dx = self._dx.get(m)
        if dx is None:
            dx = self._dx[m] = torch.empty((m, self.K), dtype=torch.float32, device=self.device)
        check(lib.y2_wide_head_backward_input(_ptr(dy), _ptr(self.packed2), m, self.K, self.Cout, float(grad_scale), _ptr(dx),
                                              _ptr(self._ws), nws, sx, _stream()))
        return dx


FP32_MAX = 3.4028234663852886e38


class WideHeadSGD:
    """Darknet's solver on a WideHead, next to DarknetSGD over the stacks of the same graph: momentum SGD, weight decay on
    W only, one launch that also rewrites both operand images (y2_wide_head_sgd_step).  `solver`: a utils.solver.Solver;
    `scaler`: the LossScaler the stacks' optimizers share, or None.  With a scaler the layer is a "next" member of the joint
    step: scan() ORs its own overflow test into the shared flag (a f16(s dy) that overflowed is an inf or NaN in dW: a
    y2_range_check over dW and db at fp32's maximum), step() uses the control block as the first member's call left it and
    never advances it.  Without one the host counts the steps and computes the rate.  accum: K * Cout + Cout slots"""

    def __init__(self, wide, solver, scaler=None):
        if solver is None:
            raise ValueError("WideHeadSGD needs Darknet's solver (utils.solver.Solver): Adam on the wide head is not built")
        self.wide, self.solver, self.scaler = wide, solver.validate(), scaler
        self._record = _lib.sgd_solver(self.solver)
        self.accum = torch.zeros(wide.K * wide.Cout + wide.Cout, dtype=torch.float32, device=wide.device)
        self.t = 0

    def scan(self):
        w = self.wide
        if self.scaler is not None and w.dW is not None:
            for g in (w.dW, w.db):
                check(w.lib.y2_range_check(_ptr(g), g.numel(), FP32_MAX, _ptr(self.scaler.ctrl), _stream()))

    def step(self, grad_mult=1.0, joint="next"):
        w = self.wide
        if w.dW is None:
            raise ValueError("WideHeadSGD.step: WideHead.backward() has not run")
        self.t += 1
        if self.scaler is not None:
            if joint != "next":
                raise ValueError("WideHeadSGD.step(joint=%r): under a shared scaler the wide head is a \"next\" member" % (joint,))
            ctrl, rate = _ptr(self.scaler.ctrl), 0.0
        else:
            r = C.c_float(0.0)
            check(w.lib.y2_solver_rate(C.byref(self._record), self.t, C.byref(r)))
            ctrl, rate = C.c_void_p(0), r.value
        check(w.lib.y2_wide_head_sgd_step(_ptr(w.W), _ptr(w.b), _ptr(self.accum), _ptr(w.dW), _ptr(w.db), w.K, w.Cout,
                                          _ptr(w.packed), w.packed.numel(), _ptr(w.packed2), w.packed2.numel(), ctrl, rate,
                                          self.solver.momentum, self.solver.decay, grad_mult, _stream()))

    def export_state(self):
        return {"accum": self.accum.cpu().numpy().copy(), "t": int(self.t)}

    def load_state(self, st):
        self.accum.copy_(torch.as_tensor(np.asarray(st["accum"], np.float32)).to(self.accum.device))
        self.t = int(st["t"])


def nms(boxes, scores, classes=None, iou_thresh=0.5, score_thresh=0.0, max_out=100, class_aware=False):
    """boxes [N,K,4], scores [N,K] (, classes [N,K] int32) -> keep [N,max_out] int32 (-1 padded), count [N]"""
    lib = _lib.load()
    n, k, _ = boxes.shape
    assert boxes.is_contiguous() and scores.is_contiguous() and scores.dtype == torch.float32
    keep = torch.empty((n, max_out), dtype=torch.int32, device=boxes.device)
    count = torch.empty((n,), dtype=torch.int32, device=boxes.device)
    cl = None
    if classes is not None:
        cl = classes.to(torch.int32).contiguous()
    check(lib.y2_nms(_ptr(boxes), _ptr(scores), _ptr(cl), n, k, float(iou_thresh), float(score_thresh), int(max_out),
                     int(bool(class_aware)), _ptr(keep), _ptr(count), _stream()))
    return keep, count


def detect_grid_batch(predict, table, index=None, num_class=20, B=2, object_thresh=0.005, iou_thresh=0.45, max_out=100,
                      out=None):
    """predict [n,S,S,num_class+5B] fp32, table int64 [entries][5] (DeviceVOC.table), index int32 [n] or None ->
    (det int32 [n,max_out,6] = xmin, ymin, xmax, ymax, class, candidate (-1 rows beyond count), score [n,max_out],
    count int32 [n]), device tensors: boxes in the 1-based pixels of each ORIGINAL image after the class-aware NMS
    (utils/detect_batch.grid_detect, bit for bit).  `out` = (det, score, count) writes into caller tensors."""
    lib = _lib.load()
    assert predict.is_cuda and predict.dtype == torch.float32 and predict.is_contiguous() and predict.dim() == 4
    n, S = predict.shape[0], predict.shape[1]
    assert tuple(predict.shape) == (n, S, S, num_class + 5 * B), predict.shape
    _entries(table, index, n, table.shape[0])
    det, score, count = _det_out(out, (n,), n, max_out, predict.device)
    check(lib.y2_detect_grid_batch(_ptr(predict), _ptr(table), _ptr(index), n, S, B, num_class, float(object_thresh),
                                   float(iou_thresh), int(max_out), _ptr(det), _ptr(score), _ptr(count), _stream()))
    return det, score, count


def _net_size(net_size, S):
    """the net_size argument of the letterboxed detect calls: the input size the head's S belongs to"""
    if int(net_size) != net_size or net_size < 32 or net_size % 32 or net_size != 32 * S:
        raise ValueError("net_size %r is not the positive multiple of 32 that S = %d makes (%d)" % (net_size, S, 32 * S))
    return int(net_size)


def _canvas(pool, table, index, n, size, dtype, out):
    """the pool / table / index contract of the letterbox and warp calls -> their output [n,size,size,3] of dtype"""
    assert pool.is_cuda and pool.dtype == torch.uint8 and pool.is_contiguous()
    _entries(table, index, n, table.shape[0])
    return _own(out, (n, size, size, 3), dtype, pool.device, n * size * size * 3)


def letterbox_batch(pool, table, index, n, size, fill=127, out=None):
    """pool uint8 [bytes], table int64 [entries][5], index int32 [n] or None (DeviceVOC's) -> out uint8 [n,size,size,3]:
    every entry letterboxed into a canvas of `fill` (img_dataset/pascal_voc.letterbox_u8, bit for bit); one launch on the
    current stream.  The batch detect_anchor_batch(..., net_size=size) un-maps."""
    out = _canvas(pool, table, index, n, size, torch.uint8, out)
    check(_lib.load().y2_letterbox_u8_batch(_ptr(pool), _ptr(table), _ptr(index), int(n), int(size), int(fill),
                                            _ptr(out), _stream()))
    return out


def warp_batch(pool, table, index, n, size, params=None, fill=127, labels=None, out=None, labels_out=None):
    """pool / table / index as letterbox_batch, params float64 [n, 9] on the device or None -> out uint8 [n,size,size,3]:
    every slot through its affine map and colour triple (img_dataset/augment_cls.ClsAugment.image, bit for bit; None: the
    plain stretch, augment_cls.plain_image).  labels int32 [entries]: also labels_out int32 [n] = labels[index], from the
    same launch, and the return value is (out, labels_out).  One launch on the current stream."""
    out = _canvas(pool, table, index, n, size, torch.uint8, out)
    if params is not None:
        assert _dev(params, torch.float64, "params").numel() >= 9 * n
    if labels is not None:
        _dev(labels, torch.int32, "labels")
        if labels_out is None:
            labels_out = torch.empty((n,), dtype=torch.int32, device=pool.device)
        assert _dev(labels_out, torch.int32, "labels_out").numel() >= n
    else:
        assert labels_out is None, "labels_out without labels"
    check(_lib.load().y2_warp_u8_batch(_ptr(pool), _ptr(table), _ptr(index), _ptr(params), _ptr(labels), int(n),
                                       int(size), int(size), int(fill), _ptr(out), _ptr(labels_out), _stream()))
    return out if labels is None else (out, labels_out)


def _detect_anchor(plain, letterboxed, per_class, net, anchors, table, index, score_thresh, iou_thresh, m, out, net_size):
    """the body of the three per-anchor detect calls: `plain` / `letterboxed` name the library's entry without and with
    net_size; rows per image (m = max_out) or per (image, class) (m = max_per_class)"""
    lib = _lib.load()
    assert net.is_cuda and net.dtype == torch.float32 and net.is_contiguous() and net.dim() == 5
    n, S, _, B, d = net.shape
    assert net.shape[2] == S and d > 5, net.shape
    C = d - 5
    an = _anchors(anchors, B, net.device)
    _entries(table, index, n, table.shape[0])
    if per_class:
        det, score, count = _det_out(out, (n, C), n * C, m, net.device)
    else:
        det, score, count = _det_out(out, (n,), n, m, net.device)
    if net_size is not None:
        check(getattr(lib, letterboxed)(_ptr(net), _ptr(an), _ptr(table), _ptr(index), n, S, B, C, float(score_thresh),
                                        float(iou_thresh), int(m), _net_size(net_size, S), _ptr(det), _ptr(score),
                                        _ptr(count), _stream()))
    else:
        check(getattr(lib, plain)(_ptr(net), _ptr(an), _ptr(table), _ptr(index), n, S, B, C, float(score_thresh),
                                  float(iou_thresh), int(m), _ptr(det), _ptr(score), _ptr(count), _stream()))
    return det, score, count


def detect_anchor_batch(net, anchors, table, index=None, score_thresh=0.005, iou_thresh=0.45, max_out=100, out=None,
                        net_size=None):
    """net [n,S,S,B,5+C] fp32 (the RAW YOLOv2 head), anchors [B,2] in cell units (a float32 device tensor, or anything
    numpy reads: uploaded here), table / index as detect_grid_batch -> the same (det, score, count): decode, class choice,
    boxes in the 1-based pixels of each ORIGINAL image and the class-aware NMS in one launch
    (utils/detect_batch.anchor_detect on decode_anchors + class_argmax of the same net, bit for bit).  net_size: the
    input was letterboxed at that size (letterbox_batch; it must be 32 S) and the boxes are un-mapped from the picture's
    rectangle (anchor_detect with net_size, y2_detect_anchor_batch_lb); None: a plain stretch"""
    return _detect_anchor("y2_detect_anchor_batch", "y2_detect_anchor_batch_lb", False, net, anchors, table, index,
                          score_thresh, iou_thresh, max_out, out, net_size)


def detect_anchor_classes_batch(net, anchors, table, index=None, score_thresh=0.005, iou_thresh=0.45, max_per_class=32,
                                out=None, net_size=None):
    """detect_anchor_batch's arguments -> (det int32 [n,C,max_per_class,6], score [n,C,max_per_class], count int32
    [n,C]): one row per (candidate, class) whose score passes, each class ordered and walked on its own, as Darknet's
    `valid` writes them (utils/detect_batch.anchor_detect_classes on decode_anchors of the same net, bit for bit).
    det.view(n * C, max_per_class, 6) with count.view(-1) and every index repeated C times is what voc_match_batch
    reads.  net_size as in detect_anchor_batch (y2_detect_anchor_classes_batch_lb)."""
    return _detect_anchor("y2_detect_anchor_classes_batch", "y2_detect_anchor_classes_batch_lb", True, net, anchors, table,
                          index, score_thresh, iou_thresh, max_per_class, out, net_size)


def _voc_match(symbol, det, score, count, boxes, counts, difficult, index, iou_thresh, out):
    """the body of voc_match_batch (integer rows) and voc_match_batch_f (float rows): one library symbol apart"""
    assert det.is_cuda and det.dtype == torch.int32 and det.is_contiguous() and det.dim() == 3 and det.shape[2] == 6
    n, max_out = det.shape[0], det.shape[1]
    assert count.dtype == torch.int32 and count.is_contiguous() and count.numel() == n
    assert score is None or (score.dtype == torch.float32 and score.is_contiguous() and score.numel() == n * max_out)
    assert boxes.is_cuda and boxes.dtype == torch.float64 and boxes.is_contiguous() and boxes.dim() == 3
    max_obj = boxes.shape[1]
    assert boxes.shape[2] == 5 and counts.dtype == torch.int32 and counts.numel() == boxes.shape[0]
    assert difficult.is_cuda and difficult.dtype == torch.uint8 and difficult.is_contiguous()
    assert tuple(difficult.shape) == (boxes.shape[0], max_obj), difficult.shape
    _entries(None, index, n, boxes.shape[0])       # no table here: without an index, the first n rows of `boxes`
    flags = torch.empty((n, max_out), dtype=torch.int32, device=det.device) if out is None else out
    assert flags.is_contiguous() and flags.dtype == torch.int32 and flags.numel() == n * max_out
    check(getattr(_lib.load(), symbol)(_ptr(det), _ptr(score), _ptr(count), _ptr(boxes), _ptr(counts), _ptr(difficult),
                                       _ptr(index), n, max_obj, max_out, float(iou_thresh), _ptr(flags), _stream()))
    return flags


def voc_match_batch(det, score, count, boxes, counts, difficult, index=None, iou_thresh=0.5, out=None):
    """det int32 [n,max_out,6], score [n,max_out], count [n] (detect_grid_batch); boxes float64 [entries,max_obj,5],
    counts int32 [entries], difficult uint8 [entries,max_obj] (DeviceVOC) -> flags int32 [n,max_out]: 1 true positive,
    0 false positive, 2 ignored, -1 beyond count (utils/detect_batch.match_image, bit for bit)"""
    return _voc_match("y2_voc_match_batch", det, score, count, boxes, counts, difficult, index, iou_thresh, out)


# ---- Darknet's test-time protocol (csrc/darknet_io.hip)
def letterbox_darknet_batch(pool, table, index, n, size, out=None):
    """letterbox_batch's pool / table / index -> out float32 [n,size,size,3], RGB in [0, 1]: every entry through Darknet's
    float letterbox_image (corner-aligned two-pass bilinear in float32, bars of 0.5;
    img_dataset/pascal_voc.letterbox_darknet, bit for bit), one launch from the uint8 pool to the network's input on the
    current stream.  The batch detect_anchor_classes_batch_darknet(..., net_size=size) un-maps."""
    out = _canvas(pool, table, index, n, size, torch.float32, out)
    check(_lib.load().y2_letterbox_darknet_batch(_ptr(pool), _ptr(table), _ptr(index), int(n), int(size), _ptr(out),
                                                 _stream()))
    return out


def detect_anchor_classes_batch_darknet(net, anchors, table, index=None, score_thresh=0.005, iou_thresh=0.45,
                                        max_per_class=32, out=None, net_size=None):
    """detect_anchor_classes_batch's arguments and outputs under Darknet's protocol, for a batch made by
    letterbox_darknet_batch at net_size (required: 32 S): the float un-map of correct_region_boxes, validity by score and
    finiteness alone, a float centre-box IoU in the walk, and rows whose words 0..3 are the BIT PATTERNS of the float32
    corners -- det[..., :4].view(torch.float32) -- so det keeps its int32 layout
    (utils/detect_batch.anchor_detect_classes_darknet on decode_anchors of the same net, bit for bit).
    voc_match_batch_f reads the [n * C] view."""
    if net_size is None:
        raise ValueError("detect_anchor_classes_batch_darknet needs net_size: Darknet's protocol is letterboxed")
    return _detect_anchor(None, "y2_detect_anchor_classes_batch_dk", True, net, anchors, table, index, score_thresh,
                          iou_thresh, max_per_class, out, net_size)


def detect_anchor_tree_batch(net, top, anchors, table, index=None, score_thresh=0.005, iou_thresh=0.45, max_out=100,
                             out=None, net_size=None, protocol="repo"):
    """detect_anchor_batch for a word-tree head, from the tree's node instead of the class row: net [n,S,S,B,5+C] fp32 (the
    RAW head: elements 0..4 of a row are read), top int32 [n*S*S*B] (word_tree_top) -> (det int32 [n,max_out,6], score
    [n,max_out], count int32 [n]).  A candidate's class is its top, its score the objectness; a top outside [0, C) (the -1
    of a skipped row) drops it.  With score_thresh >= 0 the rows are bit for bit detect_anchor_batch's on
    word_tree_head's rewrite of net (utils/detect_batch.anchor_detect(boxes, so, top, ...)).  net_size as in
    detect_anchor_batch.  protocol="darknet" (net_size required): Darknet's float un-map, float IoU and float corners as
    bit patterns in words 0..3, flat class-aware rows that voc_match_batch_f reads
    (utils/detect_batch.anchor_detect_tree_darknet).  One launch"""
    lib = _lib.load()
    if protocol not in ("repo", "darknet"):
        raise ValueError("protocol %r is neither 'repo' nor 'darknet'" % (protocol,))
    if protocol == "darknet" and net_size is None:
        raise ValueError("detect_anchor_tree_batch(protocol='darknet') needs net_size: Darknet's protocol is letterboxed")
    assert net.is_cuda and net.dtype == torch.float32 and net.is_contiguous() and net.dim() == 5
    n, S, _, B, d = net.shape
    assert net.shape[2] == S and d > 5, net.shape
    assert _dev(top, torch.int32, "top").numel() == n * S * S * B, top.shape
    an = _anchors(anchors, B, net.device)
    _entries(table, index, n, table.shape[0])
    det, score, count = _det_out(out, (n,), n, max_out, net.device)
    entry = lib.y2_detect_anchor_tree_batch_dk if protocol == "darknet" else lib.y2_detect_anchor_tree_batch
    check(entry(_ptr(net), _ptr(top), _ptr(an), _ptr(table), _ptr(index), n, S, B, d - 5, float(score_thresh),
                float(iou_thresh), int(max_out), 0 if net_size is None else _net_size(net_size, S), _ptr(det), _ptr(score),
                _ptr(count), _stream()))
    return det, score, count


def voc_match_batch_f(det, score, count, boxes, counts, difficult, index=None, iou_thresh=0.5, out=None):
    """voc_match_batch for rows whose words 0..3 hold float32 corners (detect_anchor_classes_batch_darknet):
    utils/detect_batch.match_image_f, bit for bit"""
    return _voc_match("y2_voc_match_batch_f", det, score, count, boxes, counts, difficult, index, iou_thresh, out)


# ---- COCO's bounding-box matching (csrc/coco.hip; DESIGN.md 9, "COCO evaluation")
COCO_MAX_OBJECTS, COCO_MAX_THRESHOLDS, COCO_MAX_AREAS = 256, 16, 4          # Y2_COCO_MAX_*
_coco_defaults = {}


def _coco_table(values, default, width, device):
    """thresholds / area_ranges: a float64 device tensor as it is; None: COCO's own, uploaded once per device; anything
    else numpy reads: uploaded here"""
    if torch.is_tensor(values):
        return _dev(values, torch.float64, "thresholds" if width == 1 else "area_ranges")
    if values is None:
        key = (default, str(device))
        if key not in _coco_defaults:
            from .utils import coco_eval
            _coco_defaults[key] = torch.as_tensor(np.ascontiguousarray(getattr(coco_eval, default), np.float64)).to(device)
        return _coco_defaults[key]
    return torch.as_tensor(np.ascontiguousarray(values, np.float64)).to(device)


def coco_match_batch(det, count, boxes, area, crowd, counts, index=None, thresholds=None, area_ranges=None, row_form=0,
                     out=None):
    """det int32 [n,max_out,6], count int32 [n] (the [n * C] view of detect_anchor_classes_batch's rows, or any detect
    call's); boxes float64 [entries,max_obj,5] = x, y, w, h, class in COCO's convention, area float64 [entries,max_obj],
    crowd uint8 [entries,max_obj], counts int32 [entries] (DeviceCOCO); index int32 [n] or None; thresholds float64 [T]
    and area_ranges float64 [A,2]: device tensors, anything numpy reads, or None for COCO's ten thresholds and four
    ranges -> match int32 [n,max_out,A] (`out` comes back by identity): bits 2t, 2t + 1 of word a hold 1 true positive,
    0 false positive, 2 ignored under threshold t and area range a; -1 beyond count
    (utils/coco_eval.match_segment per segment, bit for bit).  row_form 0: integer rows; 1: the float rows of
    detect_anchor_classes_batch_darknet.  One launch on the current stream.
    ValueError: "row_form R is neither 0 (integer rows) nor 1 (float rows)"; "T thresholds and A area ranges: at most 16
    and 4, and at most 64 pairs"; "max_obj = M: the matcher holds at most 256 annotations of an image"."""
    if row_form not in (0, 1):
        raise ValueError("row_form %r is neither 0 (integer rows) nor 1 (float rows)" % (row_form,))
    assert det.is_cuda and det.dtype == torch.int32 and det.is_contiguous() and det.dim() == 3 and det.shape[2] == 6
    n, max_out = det.shape[0], det.shape[1]
    assert _dev(count, torch.int32, "count").numel() == n
    assert _dev(boxes, torch.float64, "boxes").dim() == 3 and boxes.shape[2] == 5, boxes.shape
    entries, max_obj = boxes.shape[0], boxes.shape[1]
    assert tuple(_dev(area, torch.float64, "area").shape) == (entries, max_obj), area.shape
    assert tuple(_dev(crowd, torch.uint8, "crowd").shape) == (entries, max_obj), crowd.shape
    assert _dev(counts, torch.int32, "counts").numel() == entries
    _entries(None, index, n, entries)                  # no table here: without an index, the first n rows of `boxes`
    thr = _coco_table(thresholds, "THRESHOLDS", 1, det.device)
    rng = _coco_table(area_ranges, "AREA_RANGES", 2, det.device)
    assert thr.dim() == 1 and rng.dim() == 2 and rng.shape[1] == 2, (thr.shape, rng.shape)
    T, A = thr.shape[0], rng.shape[0]
    if not (1 <= T <= COCO_MAX_THRESHOLDS and 1 <= A <= COCO_MAX_AREAS and T * A <= 64):
        raise ValueError("%d thresholds and %d area ranges: at most %d and %d, and at most 64 pairs"
                         % (T, A, COCO_MAX_THRESHOLDS, COCO_MAX_AREAS))
    if max_obj > COCO_MAX_OBJECTS:
        raise ValueError("max_obj = %d: the matcher holds at most %d annotations of an image" % (max_obj, COCO_MAX_OBJECTS))
    match = _own(out, (n, max_out, A), torch.int32, det.device, n * max_out * A)
    check(_lib.load().y2_coco_match_batch(_ptr(det), _ptr(count), _ptr(boxes), _ptr(area), _ptr(crowd), _ptr(counts),
                                          _ptr(index), n, max_obj, max_out, _ptr(thr), T, _ptr(rng), A, int(row_form),
                                          _ptr(match), _stream()))
    return match


def softmax_cross_entropy(logits, labels, need_grad=True):
    """sparse_softmax_cross_entropy_with_logits + reduce_mean (imagenet_train_darknet.py:51-53)."""
    lib = _lib.load()
    logits = logits.contiguous().float()
    labels = labels.contiguous().to(torch.int32)
    n, c = logits.shape
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    dl = torch.empty_like(logits) if need_grad else None
    check(lib.y2_softmax_cross_entropy(_ptr(logits), _ptr(labels), n, c, _ptr(loss), _ptr(dl), _stream()))
    return loss, dl


def accuracy(logits, labels):
    """reduce_mean(cast(equal(argmax(logits, 1), labels))) (imagenet_train_darknet.py:60-61) -> 0-d tensor"""
    lib = _lib.load()
    logits = logits.contiguous().float()
    labels = labels.contiguous().to(torch.int32)
    n, c = logits.shape
    acc = torch.empty(1, dtype=torch.float32, device=logits.device)
    check(lib.y2_accuracy(_ptr(logits), _ptr(labels), n, c, _ptr(acc), _stream()))
    return acc[0]


def score_views(logits, labels=None, views=1, k=5, n_valid=None, hits=None, want_prob=False, top_idx=None, top_val=None,
                rank=None, prob=None):
    """logits fp32 [n * views, classes] (row b * views + v: view v of image b), labels int32 [n] or None ->
    (top_idx int32 [n, k], top_val [n, k], rank int32 [n], hits int32 [4], prob [n, classes]) as device tensors, None for
    what was not asked for (rank and hits come with labels, prob with want_prob or a `prob` tensor): softmax per view,
    mean over the views, the k best classes, the label's rank and the counters of y2_score_views in one launch on the
    current stream (utils/score_views.score_views_ref is the specification).  `hits` is ACCUMULATED: pass the tensor of
    the previous batch (None: a zeroed one); only the first n_valid images count (None: all).  top_idx, top_val, rank and
    prob may be the caller's own tensors."""
    lib = _lib.load()
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 2
    views, k = int(views), int(k)
    rows, classes = logits.shape
    if views < 1 or rows % views or rows == 0:
        raise ValueError("%d rows of logits are not a positive multiple of views = %d" % (rows, views))
    n = rows // views
    n_valid = n if n_valid is None else int(n_valid)
    dev = logits.device
    top_idx = _own(top_idx, (n, k), torch.int32, dev)
    top_val = _own(top_val, (n, k), torch.float32, dev)
    if labels is not None:
        assert _dev(labels, torch.int32, "labels").numel() == n
        rank = _own(rank, (n,), torch.int32, dev)
        hits = torch.zeros(4, dtype=torch.int32, device=dev) if hits is None else _own(hits, (4,), torch.int32, dev)
    else:
        assert rank is None and hits is None, "rank and hits need labels"
    if want_prob or prob is not None:
        prob = _own(prob, (n, classes), torch.float32, dev)
    check(lib.y2_score_views(_ptr(logits), _ptr(labels), n, views, classes, k, n_valid, _ptr(prob), _ptr(top_idx),
                             _ptr(top_val), _ptr(rank), _ptr(hits), _stream()))
    return top_idx, top_val, rank, hits, prob


def launch_log(enable=None):
    """The library's launch log (yolo2_hip.h y2_launch_log_*; host memory only).  launch_log(True) clears it and starts
    recording, launch_log(False) stops; launch_log() -> the records so far, one tuple of Y2_LAUNCH_LOG_INTS ints per
    forward / dgrad convolution (first int 0) and weight gradient (first int 1), in launch order."""
    lib = _lib.load()
    if enable is not None:
        check(lib.y2_launch_log_enable(int(bool(enable))))
        return None
    n = lib.y2_launch_log_read(None, 0)
    buf = (_lib.C.c_int * (max(n, 1) * _lib.LAUNCH_LOG_INTS))()
    n = min(n, lib.y2_launch_log_read(buf, n))
    k = _lib.LAUNCH_LOG_INTS
    return [tuple(buf[i * k:(i + 1) * k]) for i in range(n)]


def conv2d(x, w, bias=None, dtype="f32"):
    """tf.nn.conv2d(x, W, [1,1,1,1], 'SAME') (+ bias) on fp32 NHWC / HWIO device tensors."""
    lib = _lib.load()
    dt = _lib.DTYPES[dtype]
    n, h, wd, ci = x.shape
    k, _, _, co = w.shape
    x = x.contiguous().float()
    w = w.contiguous().float()
    y = torch.empty((n, h, wd, co), dtype=torch.float32, device=x.device)
    ws = torch.empty(lib.y2_conv2d_workspace_bytes(n, h, wd, ci, co, k, dt), dtype=torch.uint8, device=x.device)
    check(lib.y2_conv2d(_ptr(x), _ptr(w), _ptr(bias), _ptr(y), n, h, wd, ci, co, k, dt, _ptr(ws), _stream()))
    return y


def conv2d_backward(x, w, dy, dtype="f32", dw_out=None):
    """-> (dx, dw); dw_out: a contiguous fp32 tensor of w's size to receive dw (a view of a flat gradient buffer)"""
    lib = _lib.load()
    dt = _lib.DTYPES[dtype]
    n, h, wd, ci = x.shape
    k, _, _, co = w.shape
    x, w, dy = x.contiguous().float(), w.contiguous().float(), dy.contiguous().float()
    dx = torch.empty_like(x)
    if dw_out is not None:
        assert dw_out.is_cuda and dw_out.dtype == torch.float32 and dw_out.is_contiguous() and dw_out.numel() == w.numel()
        dw = dw_out
    else:
        dw = torch.empty_like(w)
    ws = torch.empty(lib.y2_conv2d_workspace_bytes(n, h, wd, ci, co, k, dt), dtype=torch.uint8, device=x.device)
    check(lib.y2_conv2d_backward(_ptr(x), _ptr(w), _ptr(dy), _ptr(dx), _ptr(dw), n, h, wd, ci, co, k, dt,
                                 _ptr(ws), _stream()))
    return dx, dw


# ---- operators of the ResNet-50 backbone swap (csrc/resnet_ops.hip; reference: slim_dir/nets/resnet_v1.py,
# resnet_utils.py, pascal/pascal_train_resnet.py:37-50) on fp32 NHWC device tensors -----------------------------
def batch_norm_forward(x, gamma, beta, moving_mean, moving_var, residual=None, is_training=True, update_moving=False,
                       relu=True, eps=1e-5, decay=0.997):
    """slim.batch_norm (+ residual add, + ReLU) on [..., C] -> (y, save_mean, save_var)"""
    lib = _lib.load()
    _chk(x, gamma, beta, moving_mean, moving_var, residual)
    c = x.shape[-1]
    rows = x.numel() // c
    y = torch.empty_like(x)
    sm = torch.empty(c, dtype=torch.float32, device=x.device)
    sv = torch.empty(c, dtype=torch.float32, device=x.device)
    check(lib.y2_batch_norm_forward(_ptr(x), _ptr(residual), _ptr(y), rows, c, _ptr(gamma), _ptr(beta), _ptr(moving_mean),
                                    _ptr(moving_var), _ptr(sm), _ptr(sv), float(eps), float(decay), int(is_training),
                                    int(update_moving), int(relu), _stream()))
    return y, sm, sv


def batch_norm_backward(dy, y, x, gamma, save_mean, save_var, is_training=True, relu=True, want_residual=False, eps=1e-5,
                        dgamma_out=None, dbeta_out=None):
    """-> (dx, dresidual or None, dgamma, dbeta); dgamma_out / dbeta_out: write the parameter gradients there (views
    of a flat gradient buffer)"""
    lib = _lib.load()
    _chk(dy, y, x, gamma, save_mean, save_var, dgamma_out, dbeta_out)
    c = x.shape[-1]
    rows = x.numel() // c
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_residual else None
    dg = dgamma_out if dgamma_out is not None else torch.empty(c, dtype=torch.float32, device=x.device)
    db = dbeta_out if dbeta_out is not None else torch.empty(c, dtype=torch.float32, device=x.device)
    assert dg.numel() == c and db.numel() == c
    check(lib.y2_batch_norm_backward(_ptr(dy), _ptr(y), _ptr(x), _ptr(dx), _ptr(dres), rows, c, _ptr(gamma),
                                     _ptr(save_mean), _ptr(save_var), float(eps), int(is_training), int(relu), _ptr(dg),
                                     _ptr(db), _stream()))
    return dx, dres, dg, db


def subsample(x, factor, out_hw=None):
    """resnet_utils.subsample; with out_hw=(H, W): the gradient (x at the coarse grid -> fine grid [N,H,W,C])"""
    lib = _lib.load()
    _chk(x)
    if out_hw is None:
        n, h, w, c = x.shape
        if factor == 1:
            return x
        y = torch.empty((n, (h + factor - 1) // factor, (w + factor - 1) // factor, c), dtype=torch.float32, device=x.device)
        check(lib.y2_subsample(_ptr(x), _ptr(y), n, h, w, c, int(factor), 1, _stream()))
        return y
    if factor == 1:
        return x
    n, _, _, c = x.shape
    h, w = out_hw
    y = torch.empty((n, h, w, c), dtype=torch.float32, device=x.device)
    check(lib.y2_subsample(_ptr(x), _ptr(y), n, h, w, c, int(factor), 0, _stream()))
    return y


def max_pool_3x3_s2(x):
    lib = _lib.load()
    _chk(x)
    n, h, w, c = x.shape
    y = torch.empty((n, (h + 1) // 2, (w + 1) // 2, c), dtype=torch.float32, device=x.device)
    check(lib.y2_maxpool3x3s2(_ptr(x), _ptr(y), n, h, w, c, _stream()))
    return y


def max_pool_3x3_s2_backward(x, dy):
    lib = _lib.load()
    _chk(x, dy)
    n, h, w, c = x.shape
    dx = torch.empty_like(x)
    check(lib.y2_maxpool3x3s2_backward(_ptr(x), _ptr(dy), _ptr(dx), n, h, w, c, _stream()))
    return dx


def conv7x7_s2(x, w, dtype="f32"):
    """the root block's conv2d_same(net, 64, 7, stride=2) (resnet_v1.py:197); dtype f16 / bf16: on the matrix pipe"""
    lib = _lib.load()
    _chk(x, w)
    n, h, wd, _ = x.shape
    co = w.shape[3]
    y = torch.empty((n, (h + 1) // 2, (wd + 1) // 2, co), dtype=torch.float32, device=x.device)
    check(lib.y2_conv7x7s2_t(_ptr(x), _ptr(w), _ptr(y), n, h, wd, co, _lib.DTYPES[dtype], _stream()))
    return y


def conv7x7_s2_backward_filter(x, dy, dtype="f32"):
    lib = _lib.load()
    _chk(x, dy)
    n, h, wd, _ = x.shape
    co = dy.shape[3]
    dw = torch.empty((7, 7, 3, co), dtype=torch.float32, device=x.device)
    check(lib.y2_conv7x7s2_backward_filter_t(_ptr(x), _ptr(dy), _ptr(dw), n, h, wd, co, _lib.DTYPES[dtype], _stream()))
    return dw


def fully_connected(x, w, bias=None, relu=True, dtype="f32"):
    """slim.fully_connected on [rows, in] (rows = the batch, at most 128): act(x w + bias) -> [rows, out] fp32
    (pascal_train_resnet.py:41-46); one pass over the fp32 weights (csrc/fc.hip)"""
    lib = _lib.load()
    _chk(x, w, bias)
    m, k = x.shape
    assert w.shape[0] == k
    n = w.shape[1]
    y = torch.empty((m, n), dtype=torch.float32, device=x.device)
    check(lib.y2_fully_connected(_ptr(x), _ptr(w), _ptr(bias), _ptr(y), m, k, n, int(relu), _lib.DTYPES[dtype], _stream()))
    return y


def fully_connected_backward(x, w, dz, dtype="f32", want_dx=True, dw_out=None, want_dw=True):
    """dz = gradient at the pre-activation [rows, out] -> (dx [rows, in] or None, dw [in, out] or None)"""
    lib = _lib.load()
    _chk(x, w, dz)
    m, k = x.shape
    n = w.shape[1]
    assert tuple(dz.shape) == (m, n)
    dx = torch.empty_like(x) if want_dx else None
    if not want_dw:
        check(lib.y2_fully_connected_backward(_ptr(x), _ptr(w), _ptr(dz), _ptr(dx), None, m, k, n, _lib.DTYPES[dtype], _stream()))
        return dx, None
    if dw_out is not None:
        assert dw_out.is_cuda and dw_out.dtype == torch.float32 and dw_out.is_contiguous() and dw_out.numel() == w.numel()
        dw = dw_out
    else:
        dw = torch.empty_like(w)
    check(lib.y2_fully_connected_backward(_ptr(x), _ptr(w), _ptr(dz), _ptr(dx), _ptr(dw), m, k, n, _lib.DTYPES[dtype],
                                          _stream()))
    return dx, dw


def bias_relu_(y, bias, relu=True):
    lib = _lib.load()
    _chk(y, bias)
    c = y.shape[-1]
    check(lib.y2_bias_relu(_ptr(y), _ptr(bias), y.numel() // c, c, int(relu), _stream()))
    return y


def bias_relu_backward(dy, y, relu=True, dbias_out=None):
    lib = _lib.load()
    _chk(dy, y, dbias_out)
    c = y.shape[-1]
    dz = torch.empty_like(dy)
    db = dbias_out if dbias_out is not None else torch.empty(c, dtype=torch.float32, device=dy.device)
    assert db.numel() == c
    check(lib.y2_bias_relu_backward(_ptr(dy), _ptr(y), _ptr(dz), _ptr(db), y.numel() // c, c, int(relu), _stream()))
    return dz, db


def dropout(x, keep_prob, seed):
    """tf.nn.dropout: kept elements scaled by 1/keep_prob; the same (seed) regenerates the mask for the gradient"""
    lib = _lib.load()
    _chk(x)
    y = torch.empty_like(x)
    if isinstance(seed, torch.Tensor):          # int64 [1] on the device: read by the kernel (HIP-graph replay)
        assert seed.is_cuda and seed.dtype == torch.int64 and seed.numel() == 1
        check(lib.y2_dropout_dev(_ptr(x), _ptr(y), x.numel(), float(keep_prob), _ptr(seed), _stream()))
        return y
    check(lib.y2_dropout(_ptr(x), _ptr(y), x.numel(), float(keep_prob), int(seed), _stream()))
    return y
