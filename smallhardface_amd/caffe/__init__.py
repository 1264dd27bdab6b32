"""pycaffe-compatible surface over libshf_hip.so -- exactly the subset the
reference's inference driver touches:

  caffe.set_mode_gpu / set_device / TEST      caffe/python/caffe/__init__.py:1-8, _caffe.cpp:394-396
  caffe.Net(proto, weights, phase)            _caffe.cpp:137-151,413
  net.blobs (OrderedDict, topological order)  pycaffe.py:24-32
  net.inputs / net.outputs / net.params       pycaffe.py:59-85
  net.forward(**inputs) + its two exceptions  pycaffe.py:88-134
  Blob.data (writable zero-copy fp32 view), .shape, .reshape(*dims), .count/.num/...
                                              _caffe.cpp:222-256,453-477
  Blob.device / Blob.load_device (DeviceArray) Blob::gpu_data / set_gpu_data blob.cpp:108-121, _caffe.cpp:468-470
  net.forward_group(members) / caffe.load_device_group   Net::ForwardFromTo net.cpp:516 for each of several lanes, one pass
  caffe.Layer (param_str / phase attributes)  include/caffe/layers/python_layer.hpp:27-30

Solvers, backward, forward_all, io, Classifier, NCCL are not part of the hot path.
"""
import ctypes as C
import time
from collections import OrderedDict

import numpy as np

from .. import _lib

TRAIN = 0
TEST = 1

__all__ = ["Net", "Blob", "DeviceArray", "Layer", "TEST", "TRAIN", "set_mode_gpu", "set_mode_cpu", "set_device"]


def set_mode_gpu():
    _lib.check(_lib.load().shf_set_mode_gpu(), "set_mode_gpu")


def set_mode_cpu():
    raise _lib.ShfError("smallhardface_amd is a GPU-only runtime (no CPU mode)")


def set_device(device_id):
    _lib.check(_lib.load().shf_set_device(int(device_id)), "set_device")


# arithmetic of the MFMA convolutions (C ABI shf_net_set_conv_mode): exact fp32; split-fp16 with three products
# (fp32-class: the mode every parity test runs); the reduced ladder with two / one product (drift-labelled); binary64
# accumulation with one rounding to fp32 (the on-device truth the drift of the others is measured against)
CONV_MODES = {"fp32": 0, "f16x3": 1, "f16x2": 2, "f16": 3, "bf16": 4, "f64": 5, 0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 5}
CONV_MODE_NAMES = {0: "fp32", 1: "f16x3", 2: "f16x2", 3: "f16", 4: "bf16", 5: "f64"}


class Layer(object):
    """Base class of Python layers (kept for source compatibility: the proposal
    layer runs natively inside the runtime, nothing is called back)."""
    param_str = ""
    phase = TEST

    def setup(self, bottom, top):
        pass

    def reshape(self, bottom, top):
        pass

    def forward(self, bottom, top):
        pass

    def backward(self, top, propagate_down, bottom):
        pass


_FLIP_X = (Ellipsis, slice(None, None, -1))


class DeviceArray(object):
    """An fp32, C-contiguous, 4-D NCHW block in DEVICE memory: what ``Blob.load_device`` / ``Net.forward`` take and
    ``Blob.device`` returns (pycaffe: Blob.gpu_data() / set_gpu_data()).  It holds a pointer, a shape, a reference to
    whatever owns the memory and a ``flipped`` flag -- nothing is ever copied or launched here.

    Built from any object with ``__cuda_array_interface__`` (a torch tensor on the GPU has one); a wrong dtype,
    non-contiguous strides or ``ndim != 4`` is a ValueError.  ``a[..., ::-1]`` -- the only indexing detect() needs
    (lib/test.py:150) -- returns a view with ``flipped`` toggled; the mirroring itself happens when the view is loaded
    into a blob.  While unflipped the array exposes ``__cuda_array_interface__`` itself, so
    ``torch.as_tensor(a, device="cuda")`` is zero-copy."""

    def __init__(self, src, flipped=False):
        if isinstance(src, DeviceArray):
            self.ptr, self.shape, self.owner = src.ptr, src.shape, src.owner
            self.flipped = bool(src.flipped) != bool(flipped)
            self._complete, self._blob = src._complete, src._blob
            return
        cai = getattr(src, "__cuda_array_interface__", None)
        if cai is None:
            raise TypeError("DeviceArray needs an object with __cuda_array_interface__, got %s" % type(src).__name__)
        shape = tuple(int(d) for d in cai["shape"])
        if cai.get("typestr") not in ("<f4", "=f4"):
            raise ValueError("DeviceArray holds float32, got typestr %r" % (cai.get("typestr"),))
        if len(shape) != 4:
            raise ValueError("DeviceArray holds a 4-D NCHW block, got %d axes" % len(shape))
        strides = cai.get("strides")
        if strides is not None:
            want, acc = [], 4
            for d in reversed(shape):
                want.append(acc)
                acc *= d
            # (an axis of length 1 may carry any stride)
            if any(d != 1 and int(st) != w for d, st, w in zip(shape, strides, reversed(want))):
                raise ValueError("DeviceArray needs C-contiguous memory, got strides %r for shape %r" % (tuple(strides), shape))
        self.ptr = int(cai["data"][0])
        self.shape = shape
        self.owner = src
        self.flipped = bool(flipped)
        self._complete = False    # True for a block the runtime itself produced and synchronised: no wait on torch's stream
        self._blob = None         # (net, blob index) when this is a blob's own device image (Blob.device)

    @classmethod
    def _wrap(cls, ptr, shape, owner, blob=None):
        """A block the runtime itself produced and synchronised (any number of axes: Blob.device of a 2-D blob)."""
        a = cls.__new__(cls)
        a.ptr, a.shape, a.owner, a.flipped = int(ptr), tuple(int(d) for d in shape), owner, False
        a._complete, a._blob = True, blob
        return a

    def __getitem__(self, key):
        if isinstance(key, tuple) and len(key) == 2 and key[0] is Ellipsis and key[1] == _FLIP_X[1]:
            return DeviceArray(self, flipped=True)
        raise TypeError("DeviceArray supports only a[..., ::-1] (the horizontal flip); use numpy() or torch.as_tensor() "
                        "for anything else")

    def __getattr__(self, name):
        # exposed only while unflipped: a mirrored view is not describable by (pointer, shape, positive strides)
        if name == "__cuda_array_interface__" and not self.__dict__.get("flipped", True):
            return {"shape": self.shape, "typestr": "<f4", "data": (self.ptr, False), "version": 2, "strides": None}
        raise AttributeError(name)

    @property
    def ndim(self):
        return len(self.shape)

    def numpy(self):
        """A host copy (the flip applied)."""
        import torch
        plain = DeviceArray(self, flipped=self.flipped)    # the unflipped view of the same memory
        if not self._complete:
            torch.cuda.current_stream().synchronize()
        a = torch.as_tensor(plain, device="cuda").cpu().numpy()
        return np.ascontiguousarray(a[..., ::-1]) if self.flipped else a

    def __repr__(self):
        return "DeviceArray(ptr=0x%x, shape=%r%s)" % (self.ptr, self.shape, ", flipped" if self.flipped else "")


def _resolve_source(blob, src, flip):
    """What ``src`` -- a DeviceArray or anything it accepts -- means as a device load into ``blob``: None when it is the
    blob's own device image (already in place), else (DeviceArray, the kernel's flip bit = ``flip`` XOR the source's own
    ``flipped``, whether torch's stream must be waited for first)."""
    a = src if isinstance(src, DeviceArray) else DeviceArray(src)
    if a.ndim != 4:
        raise ValueError("load_device needs a 4-D NCHW block, got shape %r" % (a.shape,))
    if a._blob is not None and a._blob[0] is blob._net and a._blob[1] == blob._i:
        if a.flipped != bool(flip):
            raise ValueError("load_device cannot mirror blob '%s' into itself: copy its device image first" % blob.name)
        return None
    return a, (1 if bool(a.flipped) != bool(flip) else 0), not a._complete


def _wait_for_torch():
    import torch
    torch.cuda.current_stream().synchronize()    # the producers' kernels: a source must be complete


class Blob(object):
    def __init__(self, net, index, name):
        self._net = net
        self._i = index
        self.name = name

    @property
    def shape(self):
        dims = (C.c_int * 8)()
        n = self._net._lib.shf_blob_shape(self._net._h, self._i, dims)
        return tuple(int(dims[i]) for i in range(n))

    def reshape(self, *dims):
        arr = (C.c_int * len(dims))(*[int(d) for d in dims])
        _lib.check(self._net._lib.shf_blob_reshape(self._net._h, self._i, arr, len(dims)), "Blob.reshape")

    @property
    def data(self):
        """Writable fp32 view of the blob's host mirror (NCHW), like mutable_cpu_data()."""
        p = self._net._lib.shf_blob_mutable_host_data(self._net._h, self._i)
        if not p:
            raise _lib.ShfError(_lib.last_error())
        shape = self.shape
        n = int(np.prod(shape)) if len(shape) else 1
        if n == 0:
            return np.zeros(shape, dtype=np.float32)
        a = np.ctypeslib.as_array(p, shape=(n,)).reshape(shape)
        a.flags.writeable = True
        self._keep = self._net  # the view borrows from the net
        return a

    @property
    def device(self):
        """The blob's fp32 NCHW image in device memory (Blob.gpu_data(), C ABI shf_blob_device_data), valid until the next
        forward, reshape or load on this net.  Tail-fused blobs have none (ShfError naming the blob): read their ``data``."""
        p = self._net._lib.shf_blob_device_data(self._net._h, self._i)
        if not p:
            raise _lib.ShfError(_lib.last_error())
        return DeviceArray._wrap(p, self.shape, self._net, blob=(self._net, self._i))

    def load_device(self, src, flip=False):
        """Blob::set_gpu_data for a net input, with forward_net's zero pad and detect()'s flip folded in (C ABI
        shf_blob_load_device): ``src`` -- a DeviceArray or anything it accepts -- of shape (n, c, h <= H, w <= W) lands in
        this (n, c, H, W) blob, mirrored along x when ``flip`` XOR the source's own ``flipped``.  The net keeps ``src``
        alive until its next forward has returned."""
        r = _resolve_source(self, src, flip)
        if r is None:
            return
        a, f, wait = r
        if wait:
            _wait_for_torch()
        n, c, h, w = a.shape
        _lib.check(self._net._lib.shf_blob_load_device(self._net._h, self._i, C.c_void_p(a.ptr), n, c, h, w, f), "Blob.load_device")
        self._net._dev_sources.append(a)

    @property
    def count(self):
        return int(np.prod(self.shape))

    num = property(lambda self: self.shape[0])
    channels = property(lambda self: self.shape[1])
    height = property(lambda self: self.shape[2])
    width = property(lambda self: self.shape[3])


class _ParamBlob(object):
    """net.params[name][i]: writing through ``.data[...]`` and calling
    ``net.commit_params()`` (or the next forward) re-packs the weights on the GPU."""

    def __init__(self, net, layer, idx):
        self._net, self._layer, self._idx = net, layer, idx

    @property
    def shape(self):
        dims = (C.c_int * 4)()
        n = self._net._lib.shf_net_param_shape(self._net._h, self._layer, self._idx, dims)
        return tuple(int(dims[i]) for i in range(n))

    @property
    def data(self):
        p = self._net._lib.shf_net_param_data(self._net._h, self._layer, self._idx)
        shape = self.shape
        self._net._dirty_layers.add(self._layer)
        return np.ctypeslib.as_array(p, shape=(int(np.prod(shape)),)).reshape(shape)


class Net(object):
    def __init__(self, network_file, weights=None, phase=TEST, prototxt_text=None):
        if isinstance(weights, int) and phase == TEST and weights in (TRAIN, TEST):
            # caffe.Net(proto, phase) 2-arg form (_caffe.cpp:152-…)
            weights, phase = None, weights
        self._lib = _lib.load()
        enc = lambda s: None if s is None else str(s).encode()
        self._h = self._lib.shf_net_create(enc(network_file), enc(prototxt_text), enc(weights or ""), int(phase))
        if not self._h:
            raise RuntimeError(_lib.last_error())
        L = self._lib
        self._blob_names = [L.shf_net_blob_name(self._h, i).decode() for i in range(L.shf_net_num_blobs(self._h))]
        self._blobs = [Blob(self, i, n) for i, n in enumerate(self._blob_names)]
        self._inputs = [L.shf_net_input_blob(self._h, i) for i in range(L.shf_net_num_inputs(self._h))]
        self._outputs = [L.shf_net_output_blob(self._h, i) for i in range(L.shf_net_num_outputs(self._h))]
        self._layer_names = [L.shf_net_layer_name(self._h, i).decode() for i in range(L.shf_net_num_layers(self._h))]
        self._layer_types = [L.shf_net_layer_type(self._h, i).decode() for i in range(L.shf_net_num_layers(self._h))]
        self._dirty_layers = set()
        self._dev_sources = []    # device sources of Blob.load_device, kept alive until the next forward has returned
        self._apply_cfg()

    @property
    def num_classes(self):
        """Classes of the proposal layer, background first (C ABI shf_net_num_classes); 0 without a proposal layer."""
        return int(self._lib.shf_net_num_classes(self._h))

    @property
    def num_modules(self):
        """Proposal layers of the net (C ABI shf_net_num_modules): one per ``boxes_<level>`` / ``cls_prob_<level>`` pair the
        driver collects (lib/test.py:67-83), 1 for the templates' single ``boxes`` / ``cls_prob``, 0 without one."""
        return int(self._lib.shf_net_num_modules(self._h))

    def clone(self):
        """A lane: same parameter tensors, own activations / workspace / HIP stream
        (cf. Net::ShareTrainedLayersWith).  Keep ``self`` alive while the lane is used."""
        self.commit_params()
        h = self._lib.shf_net_clone(self._h)
        if not h:
            raise RuntimeError(_lib.last_error())
        lane = Net.__new__(Net)
        lane._lib, lane._h, lane._parent = self._lib, h, self
        for k in ("_blob_names", "_inputs", "_outputs", "_layer_names", "_layer_types"):
            setattr(lane, k, getattr(self, k))
        lane._blobs = [Blob(lane, i, n) for i, n in enumerate(lane._blob_names)]
        lane._dirty_layers = set()
        lane._dev_sources = []
        return lane

    def _apply_cfg(self):
        """The reference's Python layer reads cfg.TEST.* at EVERY forward (lib/layers/proposal_layer.py:88-92): called
        from forward() / detect_begin(), pushed to the runtime (shared by all lanes) only when a value changed."""
        from ..config import cfg
        cur = (int(cfg.TEST.N_DETS_PER_MODULE), float(cfg.TEST.SCORE_THRESH), float(cfg.TEST.ANCHOR_MIN_SIZE))
        root = getattr(self, "_parent", self)
        if getattr(root, "_cfg_applied", None) != cur:
            self.set_proposal_cfg(*cur)
            root._cfg_applied = cur

    def set_proposal_cfg(self, pre_nms_topN, score_thresh, min_size):
        getattr(self, "_parent", self)._cfg_applied = None   # an explicit override: re-read cfg at the next forward
        _lib.check(self._lib.shf_net_set_proposal_cfg(self._h, int(pre_nms_topN), float(score_thresh),
                                                      float(min_size)), "set_proposal_cfg")

    def set_conv_mode(self, mode):
        """Arithmetic of the MFMA convolutions: "fp32" (exact fp32 MFMA), "f16x3" (split-fp16, three fp16 products per
        fp32 product: fp32-class accuracy, the parity mode), and the reduced, drift-labelled modes "f16x2", "f16" (two /
        one fp16 product; fp16 range guard applies) and "bf16" (one bf16 product; fp32's exponent range, no guard).
        "f64" accumulates every dot product (convolutions, the cls / bbox predictors, the deconvolution) in binary64 and
        rounds once to fp32: the best answer fp32 blobs can hold, for measuring the drift of the other modes on the device
        at any size.  It always runs layer by layer, as "fp32" does, and is not a throughput mode."""
        m = CONV_MODES[mode]
        self.commit_params()
        _lib.check(self._lib.shf_net_set_conv_mode(self._h, m), "set_conv_mode")

    @property
    def conv_mode(self):
        return CONV_MODE_NAMES[int(self._lib.shf_net_get_conv_mode(self._h))]

    def set_layer_products(self, table):
        """{layer name: 1 | 2 | 3 (0 clears)}: fp16 products per fp32 product for single layers of a split-fp16 mode
        (C ABI shf_net_set_layer_products)."""
        for name, n in dict(table).items():
            _lib.check(self._lib.shf_net_set_layer_products(self._h, str(name).encode(), int(n)), "set_layer_products")

    @property
    def range_fallbacks(self):
        """Forwards this net (and its lanes) re-ran on the exact fp32 kernels because a split-fp16 convolution left
        the fp16 range (C ABI shf_net_range_fallbacks)."""
        return int(self._lib.shf_net_range_fallbacks(self._h))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.shf_net_destroy(h)

    # -- pycaffe.py:24-85 ------------------------------------------------------
    @property
    def blobs(self):
        if not hasattr(self, "_blobs_dict"):
            self._blobs_dict = OrderedDict(zip(self._blob_names, self._blobs))
        return self._blobs_dict

    @property
    def params(self):
        if not hasattr(self, "_params_dict"):
            d = OrderedDict()
            for li, name in enumerate(self._layer_names):
                n = self._lib.shf_net_layer_num_params(self._h, li)
                if n > 0:
                    d[name] = [_ParamBlob(self, li, i) for i in range(n)]
            self._params_dict = d
        return self._params_dict

    @property
    def inputs(self):
        return [self._blob_names[i] for i in self._inputs]

    @property
    def outputs(self):
        return [self._blob_names[i] for i in self._outputs]

    def commit_params(self):
        for li in sorted(self._dirty_layers):
            _lib.check(self._lib.shf_net_param_commit(self._h, li), "param_commit")
        self._dirty_layers.clear()

    def _stage_inputs(self, kwargs, deferred=None):
        """forward(**kwargs)'s checks and input copies (pycaffe.py:108-117).  ``deferred`` (forward_group): a device input is
        not loaded here but appended as (net, input name, DeviceArray), for one grouped load of all members."""
        if set(kwargs.keys()) != set(self.inputs):
            raise Exception('Input blob arguments do not match net inputs.')
        for in_, blob in kwargs.items():
            if not isinstance(blob, (np.ndarray, DeviceArray)) and hasattr(blob, "__cuda_array_interface__"):
                blob = DeviceArray(blob)    # e.g. a torch tensor on the GPU
            if blob.shape[0] != self.blobs[in_].shape[0]:
                raise Exception('Input is not batch sized')
            if isinstance(blob, DeviceArray):
                b = self.blobs[in_]
                if tuple(blob.shape) != tuple(b.shape):
                    fmt = lambda sh: "(%s)" % ",".join(str(int(d)) for d in sh)
                    raise ValueError("could not broadcast input array from shape %s into shape %s"
                                     % (fmt(blob.shape), fmt(b.shape)))
                # (the blob's own device image -- test.forward_net after Blob.load_device -- is already in place)
                own = (not blob.flipped and blob._blob is not None and blob._blob[0] is self
                       and blob._blob[1] == b._i and blob.ptr == b.device.ptr)
                if not own:
                    if deferred is not None:
                        deferred.append((self, in_, blob))
                    else:
                        b.load_device(blob)
                continue
            dst = self.blobs[in_].data
            # (a caller that filled the blob's own host mirror in place -- test.forward_net -- hands that view back)
            if not (isinstance(blob, np.ndarray) and blob.ctypes.data == dst.ctypes.data and blob.shape == dst.shape
                    and blob.strides == dst.strides):
                dst[...] = blob

    def _run_forward(self, members, inputs, names, group):
        """forward() of ``members`` with ``self`` as the head: ``inputs[k]`` (None or forward's kwargs) staged into
        ``members[k]``, one call, {name: Blob.data} of ``names(member)`` per member.  ``group``: the device inputs go in with
        one grouped load per input name and the call is shf_net_forward_group; else Blob.load_device and shf_net_forward."""
        tm = getattr(self, "timing", None)     # measurement only (bench.py net_forward_path): a dict collects host seconds
        now = time.perf_counter if tm is not None else (lambda: 0.0)
        t0 = now()
        self.commit_params()
        self._apply_cfg()
        try:
            deferred = [] if group else None
            for m, kw in zip(members, inputs):
                if kw:
                    m._stage_inputs(kw, deferred)
            for name in sorted(set(d[1] for d in deferred or ())):
                sel = [d for d in deferred if d[1] == name]
                _load_device_group(self, [d[0] for d in sel], name, [d[2] for d in sel], None)
            t1 = now()
            if group:
                n = len(members)
                mem = (C.c_void_p * max(n, 1))(*[getattr(m, "_h", None) for m in members])
                _lib.check(self._lib.shf_net_forward_group(self._h, n, mem), "Net.forward_group")
            else:
                _lib.check(self._lib.shf_net_forward(self._h), "Net.forward")
        finally:
            for m in members:       # (the call synchronises: the loads' kernels are done with their sources)
                if isinstance(m, Net):
                    del m._dev_sources[:]
        t2 = now()
        out = [{o: m.blobs[o].data for o in names(m)} for m in members]
        if tm is not None:
            t3 = now()
            tm["calls"] = tm.get("calls", 0) + 1
            if group:
                tm["units"] = tm.get("units", 0) + len(members)
            tm["input_copy_s"] = tm.get("input_copy_s", 0.0) + (t1 - t0)     # host blob -> the pinned mirror (Blob.data[...] = x), or a DeviceArray's load
            tm["forward_call_s"] = tm.get("forward_call_s", 0.0) + (t2 - t1)  # shf_net_forward(_group): H2D + kernels + the count read-back
            tm["output_read_s"] = tm.get("output_read_s", 0.0) + (t3 - t2)   # Blob.data of the outputs: D2H
        return out

    def forward(self, blobs=None, start=None, end=None, **kwargs):
        """pycaffe.py:88-134 (whole-net forward only: start/end are not supported)."""
        if start is not None or end is not None:
            raise NotImplementedError("partial forward (start/end) is outside the inference hot path")
        return self._run_forward([self], [kwargs], lambda m: set(m.outputs + (blobs or [])), False)[0]

    def _forward(self):
        """forward() on the blobs as they stand, no output read (tools/bench_conv.py, tools/bench_one.py)."""
        self._run_forward([self], [None], lambda m: (), False)

    def forward_group(self, members, inputs=None):
        """``forward()`` of several nets as ONE grouped pass (C ABI shf_net_forward_group): every convolution, the
        deconvolution and every stage of the proposal tail is one launch over the group, whatever the members' sizes -- the
        levels of a pyramid in one pass.  ``members``: a list of distinct nets, ``self`` and / or lanes from ``self.clone()``
        (at most 16); ``self`` is the head, whose stream carries the pass.  ``inputs``: None (the members' input blobs as
        they stand) or one entry per member, each None or a dict of what ``forward(**kwargs)`` accepts -- numpy arrays,
        DeviceArray, anything with ``__cuda_array_interface__`` --, under forward()'s checks and exception texts; the
        device inputs of all members go in with one launch per input name.  Returns a list of {output name: Blob.data},
        one per member.  Afterwards every member is an ordinary forwarded net: its results are bit for bit those of its
        own ``forward()``, and every blob of it reads as after one."""
        members = list(members)
        inputs = [None] * len(members) if inputs is None else list(inputs)
        if len(inputs) != len(members):
            raise ValueError("forward_group: %d members but %d input dicts" % (len(members), len(inputs)))
        return self._run_forward(members, inputs, lambda m: m.outputs, True)

    def handover_event(self):
        """(waits, holds) of C ABI shf_debug_handover_event: whether a later grouped pass over this net as a member lane
        waits for an event, and whether this net keeps that event alive (tests)."""
        w, h = C.c_int(0), C.c_int(0)
        _lib.check(self._lib.shf_debug_handover_event(self._h, C.byref(w), C.byref(h)), "debug_handover_event")
        return bool(w.value), bool(h.value)

    # -- measurement helpers ------------------------------------------------------
    def sync(self):
        _lib.check(self._lib.shf_net_sync(self._h), "sync")

    def prof_enable(self, on=True):
        self._lib.shf_prof_enable(self._h, 1 if on else 0)

    def prof_only(self, class_name=None):
        """Bracket only launches of the named kernel class (None: every class) -- C ABI shf_prof_only."""
        cls = -1
        if class_name is not None:
            names = [self._lib.shf_prof_class_name(self._h, c).decode() for c in range(self._lib.shf_prof_num_classes(self._h))]
            cls = names.index(class_name)
        self._lib.shf_prof_only(self._h, cls)

    def prof_reset(self):
        _lib.check(self._lib.shf_prof_reset(self._h), "prof_reset")

    def prof_read(self):
        out = OrderedDict()
        for c in range(self._lib.shf_prof_num_classes(self._h)):
            n, ms, fl, by = C.c_int64(), C.c_double(), C.c_double(), C.c_double()
            _lib.check(self._lib.shf_prof_read(self._h, c, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)))
            out[self._lib.shf_prof_class_name(self._h, c).decode()] = dict(
                launches=n.value, ms=ms.value, flops=fl.value, bytes=by.value)
        return out

    # -- fused per-image path (device-resident pyramid) ----------------------------
    def detect_begin(self):
        self.commit_params()
        self._apply_cfg()
        _lib.check(self._lib.shf_detect_begin(self._h), "detect_begin")

    def detect_add_level(self, data, H, W, im_h, im_w, im_scale, flip, thresh, on_device=False):
        """``data``: device pointer (int) when on_device else a C-contiguous fp32 (1,3,H,W) array."""
        if on_device:
            ptr = C.c_void_p(int(data))
        else:
            data = np.ascontiguousarray(data, dtype=np.float32)
            ptr = data.ctypes.data_as(C.c_void_p)
        _lib.check(self._lib.shf_detect_add_level(self._h, ptr, 1 if on_device else 0, int(H), int(W), int(im_h),
                                                  int(im_w), float(im_scale), 1 if flip else 0, float(thresh)),
                   "detect_add_level")

    def detect_add_levels(self, members, units, thresh, on_device=False, per_member_lists=False):
        """One grouped pass over several units (C ABI shf_detect_add_levels).  ``members``: distinct
        nets (self and/or lanes) lending their activation buffers, one per unit."""
        n = len(units)
        keep = []
        ptrs = (C.c_void_p * n)()
        for i, u in enumerate(units):
            if on_device:
                ptrs[i] = int(u[0])
            else:
                a = np.ascontiguousarray(u[0], dtype=np.float32)
                keep.append(a)
                ptrs[i] = a.ctypes.data
        mem = (C.c_void_p * n)(*[m._h for m in members[:n]])
        ia = lambda k: (C.c_int * n)(*[int(u[k]) for u in units])
        sc = (C.c_float * n)(*[float(u[5]) for u in units])
        fl = (C.c_int * n)(*[1 if u[6] else 0 for u in units])
        _lib.check(self._lib.shf_detect_add_levels(self._h, n, mem, ptrs, 1 if on_device else 0, ia(1), ia(2),
                                                   ia(3), ia(4), sc, fl, float(thresh),
                                                   1 if per_member_lists else 0), "detect_add_levels")

    def make_pyramid_level(self, im_dev, im_h, im_w, scale, flip, pixel_means, out_dev, H, W, lvl_h, lvl_w):
        """_get_image_blob + flip + pad for one unit on this net's stream (C ABI shf_make_pyramid_level):
        ``im_dev`` raw BGR uint8 HxWx3 device pointer -> ``out_dev`` (1,3,H,W) fp32 device pointer."""
        pm = (C.c_double * 3)(*[float(v) for v in np.asarray(pixel_means).reshape(-1)[:3]])
        _lib.check(self._lib.shf_make_pyramid_level(self._h, int(im_dev), int(im_h), int(im_w), float(scale),
                                                    1 if flip else 0, pm, int(out_dev), int(H), int(W), int(lvl_h),
                                                    int(lvl_w)), "make_pyramid_level")

    def set_predecessor(self, prev):
        """Pipeline hand-over at logits granularity (C ABI shf_net_set_predecessor)."""
        _lib.check(self._lib.shf_net_set_predecessor(self._h, prev._h if prev is not None else None), "set_predecessor")

    def set_pipeline(self, enable=True):
        """Shared in-order conv stream + high-priority own stream for this head (C ABI shf_net_set_pipeline)."""
        _lib.check(self._lib.shf_net_set_pipeline(self._h, 1 if enable else 0), "set_pipeline")

    def record_event(self):
        _lib.check(self._lib.shf_net_record_event(self._h), "record_event")

    def wait_event(self, other):
        _lib.check(self._lib.shf_net_wait_event(self._h, other._h), "wait_event")

    def detect_count(self):
        n = self._lib.shf_detect_count(self._h)
        if n < 0:
            raise _lib.ShfError(_lib.last_error())
        return n

    def detect_export(self, dst_ptr, cap_rows):
        """Copy this image's rows to a device buffer (e.g. a torch tensor's data_ptr()); returns the row count."""
        n = C.c_int(0)
        _lib.check(self._lib.shf_detect_export(self._h, C.c_void_p(int(dst_ptr)), int(cap_rows), C.byref(n)),
                   "detect_export")
        return n.value

    def detect_export_many(self, members, dst_ptrs, cap_rows):
        """Row counts of the members' lists after a per_member_lists pass; rows land in dst_ptrs[m]."""
        n = len(members)
        mem = (C.c_void_p * n)(*[m._h for m in members])
        dst = (C.c_void_p * n)(*[int(p) for p in dst_ptrs])
        cnt = (C.c_int * n)()
        _lib.check(self._lib.shf_detect_export_many(self._h, n, mem, dst, int(cap_rows), cnt), "detect_export_many")
        return [int(cnt[i]) for i in range(n)]

    def detect_import(self, src_ptr, n_rows):
        _lib.check(self._lib.shf_detect_import(self._h, C.c_void_p(int(src_ptr)), int(n_rows)), "detect_import")

    # -- per-class lists of a multi-class image (C ABI shf_class_lists_*) ---------------
    def class_lists_begin(self):
        """Empty this net's per-class detection lists: one per foreground class, resident on the device."""
        self.commit_params()
        self._apply_cfg()
        _lib.check(self._lib.shf_class_lists_begin(self._h), "class_lists_begin")

    def class_lists_add(self, members, im_w, im_scale, flip, thresh):
        """Append the outputs of ``members`` -- nets that have completed ``forward()`` / ``forward_group``, at most 16 --
        to the lists: per member forward_net's flip fix about ``im_w[i]`` when ``flip[i]`` and the division by
        ``im_scale[i]``, then every row with ``cls_prob[r, c] > thresh`` to the list of class c, in (member, row) order.
        Read from the members' device buffers; runs on this net's stream."""
        members = list(members)
        n = len(members)
        if not (len(im_w) == len(im_scale) == len(flip) == n):
            raise ValueError("class_lists_add: %d members, %d widths, %d scales, %d flips" % (n, len(im_w), len(im_scale), len(flip)))
        mem = (C.c_void_p * max(n, 1))(*[getattr(m, "_h", None) for m in members])
        _lib.check(self._lib.shf_class_lists_add(self._h, n, mem, (C.c_int * max(n, 1))(*[int(v) for v in im_w]),
                                                 (C.c_float * max(n, 1))(*[float(v) for v in im_scale]),
                                                 (C.c_int * max(n, 1))(*[1 if v else 0 for v in flip]), float(thresh)),
                   "class_lists_add")

    def debug_class_lists_add(self, boxes5, probs, im_w, im_scale, flip, thresh):
        """``class_lists_add`` on injected host arrays (C ABI shf_debug_class_lists_add): per unit ``boxes5[i]`` (R_i, 5)
        and ``probs[i]`` (R_i, C), C = ``self.num_classes``."""
        nc = self.num_classes
        bs = [np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 5) for b in boxes5]
        ps = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1, nc) for p in probs]
        n = len(bs)
        if not (len(ps) == len(im_w) == len(im_scale) == len(flip) == n):
            raise ValueError("debug_class_lists_add: %d boxes, %d probs, %d widths, %d scales, %d flips"
                             % (n, len(ps), len(im_w), len(im_scale), len(flip)))
        # (a unit without score rows keeps the layer's dummy roi in boxes5: R is the number of SCORE rows)
        R = [len(p) for p in ps]
        assert all(len(b) >= r for b, r in zip(bs, R))
        k = max(n, 1)
        _lib.check(self._lib.shf_debug_class_lists_add(
            self._h, n, (C.c_void_p * k)(*[b.ctypes.data for b in bs]), (C.c_void_p * k)(*[p.ctypes.data for p in ps]),
            (C.c_int * k)(*R), (C.c_int * k)(*[int(v) for v in im_w]), (C.c_float * k)(*[float(v) for v in im_scale]),
            (C.c_int * k)(*[1 if v else 0 for v in flip]), float(thresh)), "debug_class_lists_add")

    def class_lists_count(self):
        """Rows of each foreground class's list, class 1 first."""
        n = max(self.num_classes - 1, 1)
        cnt = (C.c_int * n)()
        _lib.check(self._lib.shf_class_lists_count(self._h, cnt), "class_lists_count")
        return [int(cnt[i]) for i in range(self.num_classes - 1)]

    def class_lists_export(self, cls, dst_ptr=None, cap_rows=0):
        """The rows of class ``cls`` (1 .. C-1): copied to the device buffer ``dst_ptr`` (``cap_rows`` rows; returns the
        list's row count), or with ``dst_ptr=None`` returned as a float32 (n, 5) host array (tests)."""
        if dst_ptr is not None:
            n = self._lib.shf_class_lists_export(self._h, int(cls), C.c_void_p(int(dst_ptr)), int(cap_rows))
            if n < 0:
                raise _lib.ShfError("class_lists_export: " + _lib.last_error())
            return n
        import torch
        n = self._lib.shf_class_lists_export(self._h, int(cls), None, 0)
        if n < 0:
            raise _lib.ShfError("class_lists_export: " + _lib.last_error())
        buf = torch.empty((max(n, 1), 5), dtype=torch.float32, device="cuda")
        m = self._lib.shf_class_lists_export(self._h, int(cls), C.c_void_p(buf.data_ptr()), n)
        if m != n:
            raise _lib.ShfError("class_lists_export: " + (_lib.last_error() if m < 0 else "the list changed under the export"))
        return buf[:n].cpu().numpy()

    def class_lists_finish(self, cls, method="BBOX_VOTE", nms_thresh=0.4, count=None):
        """The merged boxes of class ``cls`` as detect() returns them: float64 (M, 5) for "BBOX_VOTE" (bbox_vote's
        result), float32 ``dets[keep]`` rows for "NMS".  ``count``: the class's row count when the caller already has it
        (class_lists_count), sizing the output without another read."""
        m = {"BBOX_VOTE": 0, "NMS": 1}[method]
        cap = max(int(self.class_lists_count()[int(cls) - 1] if count is None and 1 <= int(cls) < self.num_classes
                      else (count or 0)), 1)
        out = np.empty((cap, 5), dtype=np.float64)
        n = C.c_int(0)
        _lib.check(self._lib.shf_class_lists_finish(self._h, int(cls), m, float(nms_thresh),
                                                    out.ctypes.data_as(C.POINTER(C.c_double)), cap, C.byref(n)),
                   "class_lists_finish")
        if n.value > cap:
            raise _lib.ShfError("class_lists_finish: %d merged rows from a list of %d" % (n.value, cap))
        return out[:n.value].copy() if m == 0 else out[:n.value].astype(np.float32)

    # -- diagnostics (tests) -----------------------------------------------------------
    def debug_proposal(self, scores, deltas, im_info):
        """ProposalLayer.forward on injected blobs through the HIP tail (C ABI shf_debug_proposal):
        scores (1,C*A,h,w), deltas (1,4A,h,w), im_info (1,3) -> (boxes (max(R,1),5), probs (R,C), overflow flag),
        C = ``self.num_classes``."""
        sc = np.ascontiguousarray(scores, dtype=np.float32)
        dl = np.ascontiguousarray(deltas, dtype=np.float32)
        ii = np.ascontiguousarray(im_info, dtype=np.float32).reshape(-1)
        h, w = sc.shape[2:]
        nc = self.num_classes
        A = sc.shape[1] // nc
        assert sc.shape[1] == nc * A and dl.shape == (1, 4 * A, h, w), (sc.shape, dl.shape, nc)
        cap = h * w * A
        boxes = np.zeros((cap, 5), np.float32)
        probs = np.zeros((cap, nc), np.float32)
        n, of = C.c_int(0), C.c_int(0)
        F = C.POINTER(C.c_float)
        _lib.check(self._lib.shf_debug_proposal(self._h, sc.ctypes.data_as(F), dl.ctypes.data_as(F), h, w,
                                                ii.ctypes.data_as(F), boxes.ctypes.data_as(F), probs.ctypes.data_as(F),
                                                cap, C.byref(n), C.byref(of)), "debug_proposal")
        return boxes[:max(n.value, 1)].copy(), probs[:n.value].copy(), bool(of.value)

    def debug_append(self, boxes5, probs2, im_w, im_scale, flip, thresh):
        """forward_net's flip fix / unscale + the > thresh cut on injected proposals (C ABI shf_debug_append)."""
        b = np.ascontiguousarray(boxes5, dtype=np.float32).reshape(-1, 5)
        p = np.ascontiguousarray(probs2, dtype=np.float32).reshape(-1, 2)
        assert len(b) == len(p)
        F = C.POINTER(C.c_float)
        _lib.check(self._lib.shf_debug_append(self._h, b.ctypes.data_as(F), p.ctypes.data_as(F), len(b), int(im_w),
                                              float(im_scale), 1 if flip else 0, float(thresh)), "debug_append")

    def detect_finish(self, method="BBOX_VOTE", nms_thresh=0.4, cap=None):
        m = {"BBOX_VOTE": 0, "NMS": 1}[method]
        cap = cap or 4096
        while True:
            out = np.empty((cap, 5), dtype=np.float64)
            n = C.c_int(0)
            _lib.check(self._lib.shf_detect_finish(self._h, m, float(nms_thresh),
                                                   out.ctypes.data_as(C.POINTER(C.c_double)), cap, C.byref(n)),
                       "detect_finish")
            if n.value <= cap:
                return out[:n.value]
            cap = n.value  # rare: more merged boxes than expected -> the merge is re-run


def _load_device_group(head, nets, name, sources, flips):
    nets, sources = list(nets), list(sources)
    flips = [False] * len(nets) if flips is None else list(flips)
    if not (len(nets) == len(sources) == len(flips)):
        raise ValueError("load_device_group: %d nets, %d sources, %d flips" % (len(nets), len(sources), len(flips)))
    todo, wait = [], False
    for i, (net, src, flip) in enumerate(zip(nets, sources, flips)):
        b = net.blobs[name]
        r = _resolve_source(b, src, flip)
        if r is None:
            continue
        a, f, w = r
        shp = b.shape
        if len(shp) == 4 and tuple(a.shape[:2]) != tuple(shp[:2]):    # (the C entry takes n and c from the blob itself)
            raise _lib.ShfError("load_device_group: member %d: blob_load_device: blob '%s' is (%d, %d, ...), the source (%d, %d, ...)"
                                % (i, b.name, shp[0], shp[1], a.shape[0], a.shape[1]))
        wait = wait or w
        todo.append((net, b._i, a, f))
    if not todo:
        return
    if len(set(t[1] for t in todo)) != 1:
        raise ValueError("load_device_group: the nets do not hold blob '%s' at the same index (not lanes of one net)" % name)
    if wait:
        _wait_for_torch()
    n = len(todo)
    mem = (C.c_void_p * n)(*[t[0]._h for t in todo])
    src = (C.c_void_p * n)(*[t[2].ptr for t in todo])
    ia = lambda v: (C.c_int * n)(*[int(x) for x in v])
    _lib.check(head._lib.shf_blob_load_device_group(head._h, n, mem, todo[0][1], src, ia(t[2].shape[2] for t in todo),
                                                    ia(t[2].shape[3] for t in todo), ia(t[3] for t in todo)),
               "load_device_group")
    for net, _, a, _f in todo:
        net._dev_sources.append(a)


def load_device_group(nets, name, sources, flips=None):
    """``Blob.load_device`` for input blob ``name`` of several nets -- lanes of one net -- in ONE launch (C ABI
    shf_blob_load_device_group), enqueued on the first net's stream: ``sources[i]`` (a DeviceArray or anything it accepts,
    (n, c, h <= H, w <= W)) lands in ``nets[i].blobs[name]``, mirrored along x when ``flips[i]`` XOR the source's own
    ``flipped``.  Blob.load_device's rules hold per net: a blob's own device image is left in place (and cannot be
    mirrored into itself), torch's stream is waited for when a source is not known to be complete, and each net keeps
    its source alive until its next forward has returned."""
    nets = list(nets)
    if not nets:
        raise ValueError("load_device_group: no nets")
    _load_device_group(nets[0], nets, name, sources, flips)


def pyramid_level_shape(im_h, im_w, scale, max_resolution):
    """(lvl_h, lvl_w, H, W) of one pyramid unit (C ABI shf_pyramid_level_shape; needs no GPU)."""
    lib = _lib.load(require_gpu=False)
    o = [C.c_int() for _ in range(4)]
    if lib.shf_pyramid_level_shape(int(im_h), int(im_w), float(scale), int(max_resolution), *[C.byref(v) for v in o]):
        raise ValueError("pyramid_level_shape: bad geometry %r" % ((im_h, im_w, scale, max_resolution),))
    return tuple(v.value for v in o)


def alloc_counts():
    """(device, pinned host) (re)allocations the runtime's grow-only buffers have made in this process so far
    (C ABI shf_alloc_counts): unchanged by a stream of images whose shapes were all seen before."""
    lib = _lib.load(require_gpu=False)
    d, h = C.c_longlong(0), C.c_longlong(0)
    lib.shf_alloc_counts(C.byref(d), C.byref(h))
    return int(d.value), int(h.value)
