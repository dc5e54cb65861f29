"""Engine — thin Python handle on a bgs_engine (include/bgs_hip.h), used by tests and bench.py.

Two call shapes, mirroring the two C entry points:
  process(frame)            host numpy frame in, (mask, background) out   == IBGS::process (package_bgs/IBGS.h:24)
  process_batch_device(...) torch CUDA tensors, asynchronous, all streams == the roofline path
numpy/torch only carry memory here; all arithmetic happens inside libbgs_hip.
"""
import ctypes as C

import numpy as np

from . import capi


class Engine:
    def __init__(self, algo, params=None, device=0, n_streams=1):
        self._h = C.c_void_p()
        self.algo = algo
        self.n_streams = n_streams
        self.params = params if params is not None else capi.default_params(algo)
        capi.check(capi.lib().bgs_create(algo, C.byref(self.params), device, n_streams, C.byref(self._h)))

    @classmethod
    def from_handle(cls, handle, algo, n_streams):
        """A view of a bgs_engine owned by someone else (a bgs_node's per-device engine): close() does not destroy it."""
        self = cls.__new__(cls)
        self._h, self.algo, self.n_streams, self.params, self._borrowed = handle, algo, n_streams, capi.default_params(algo), True
        return self

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            if not getattr(self, "_borrowed", False):
                capi.lib().bgs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- configuration ------------------------------------------------------
    def set_params(self, params):
        capi.check(capi.lib().bgs_set_params(self._h, C.byref(params)))
        self.params = params

    # set_<name>_params(params=None, **kw) / get_<name>_params() of every capi.PARAM_BLOCKS row are made from these two below the class
    def _set_block_params(self, b, params, kw):
        if params is None:
            params = self._get_block_params(b)
        for k, v in kw.items():
            setattr(params, k, v)
        capi.check(getattr(capi.lib(), "bgs_set_%s_params" % b.name)(self._h, C.byref(params)))

    def _get_block_params(self, b):
        p = b.struct()
        capi.check(getattr(capi.lib(), "bgs_get_%s_params" % b.name)(self._h, C.byref(p)))
        return p

    def set_option(self, option, value):
        capi.check(capi.lib().bgs_set_option(self._h, option, int(value)))

    def set_ingest(self, cfg):
        """bgs_set_ingest: process() then takes raw captured frames and returns outputs in the prepared geometry."""
        capi.check(capi.lib().bgs_set_ingest(self._h, C.byref(cfg) if cfg is not None else None))
        self._ingest = cfg

    def set_geometry(self, rows, cols, channels):
        capi.check(capi.lib().bgs_set_geometry(self._h, rows, cols, channels))

    # -- host path (IBGS::process) -------------------------------------------
    def process(self, frame, stream=0, want_bg=True):
        """frame: HxW or HxWxC uint8 (any row stride).  Returns (mask or None, background or None):
        None where the reference leaves the output untouched (warm-up frames, classes that write no background)."""
        if frame is None or frame.size == 0:
            flags = C.c_uint32(0)
            capi.check(capi.lib().bgs_process(self._h, stream, None, 0, 0, 3, 0, None, 0, None, 0, C.byref(flags)))
            return None, None
        assert frame.dtype == np.uint8
        rows, cols = frame.shape[:2]
        ch = 1 if frame.ndim == 2 else frame.shape[2]
        if frame.strides[-1] != 1 or (frame.ndim == 3 and frame.strides[1] != ch):
            frame = np.ascontiguousarray(frame)
        step = frame.strides[0]
        in_rows, in_cols = rows, cols
        if getattr(self, "_ingest", None) is not None:  # outputs come out in the prepared geometry
            r, c = C.c_int(0), C.c_int(0)
            capi.check(capi.lib().bgs_ingest_size(C.byref(self._ingest), rows, cols, C.byref(r), C.byref(c)))
            rows, cols = r.value, c.value
        fg = np.empty((rows, cols), np.uint8)
        bg_ch = 1 if self.algo in (capi.ASBL, capi.VUMETER) else ch
        bg = np.empty((rows, cols, bg_ch), np.uint8) if want_bg else None
        flags = C.c_uint32(0)
        capi.check(capi.lib().bgs_process(
            self._h, stream, frame.ctypes.data_as(C.c_void_p), in_rows, in_cols, ch, step,
            fg.ctypes.data_as(C.c_void_p), cols,
            bg.ctypes.data_as(C.c_void_p) if bg is not None else None, cols * bg_ch, C.byref(flags)))
        f = flags.value
        if bg is not None and bg_ch == 1:
            bg = bg[:, :, 0]
        return (fg if f & capi.FG_VALID else None), (bg if (bg is not None and f & capi.BG_VALID) else None)

    def process_into(self, frame, fg, bg=None, stream=0):
        """bgs_process into caller-owned arrays (contiguous): what a caller that keeps its images allocated does; with
        OPT_HOST_REGISTER the same buffers are page-locked once and DMA'd in place.  Returns the out_flags."""
        rows, cols = frame.shape[:2]
        ch = 1 if frame.ndim == 2 else frame.shape[2]
        flags = C.c_uint32(0)
        capi.check(capi.lib().bgs_process(self._h, stream, frame.ctypes.data_as(C.c_void_p), rows, cols, ch, frame.strides[0], fg.ctypes.data_as(C.c_void_p), fg.strides[0],
                                          bg.ctypes.data_as(C.c_void_p) if bg is not None else None, bg.strides[0] if bg is not None else 0, C.byref(flags)))
        return flags.value

    def submit(self, frame, fg, bg=None, stream=0):
        """bgs_submit: queue one frame of `stream` (caller-owned contiguous arrays, valid until wait())."""
        rows, cols = frame.shape[:2]
        ch = 1 if frame.ndim == 2 else frame.shape[2]
        capi.check(capi.lib().bgs_submit(self._h, stream, frame.ctypes.data_as(C.c_void_p), rows, cols, ch, frame.strides[0], fg.ctypes.data_as(C.c_void_p), fg.strides[0],
                                         bg.ctypes.data_as(C.c_void_p) if bg is not None else None, bg.strides[0] if bg is not None else 0))

    def host_arena(self, array, on=True):
        """bgs_host_arena: page-lock a numpy array that holds the images of several cameras, once."""
        capi.check(capi.lib().bgs_host_arena(self._h, array.ctypes.data_as(C.c_void_p), array.nbytes, 1 if on else 0))

    def wait(self, stream=0):
        flags = C.c_uint32(0)
        capi.check(capi.lib().bgs_wait(self._h, stream, C.byref(flags)))
        return flags.value

    def process_mask_only_on_device(self, frame, stream=0):
        """bgs_process with fg = bg = NULL: the mask stays on the device (for last_mask_blobs).  Returns the out_flags."""
        rows, cols = frame.shape[:2]
        ch = 1 if frame.ndim == 2 else frame.shape[2]
        frame = np.ascontiguousarray(frame)
        flags = C.c_uint32(0)
        capi.check(capi.lib().bgs_process(self._h, stream, frame.ctypes.data_as(C.c_void_p), rows, cols, ch, frame.strides[0], None, 0, None, 0, C.byref(flags)))
        return flags.value

    def last_mask_blobs(self, stream=0, connectivity=8, min_w=0, min_h=0, max_boxes=4096):
        """bgs_last_mask_blobs: (boxes int32 [k][6] = BOX_FIELDS, moments int64 [k][4] = sx, sy, sxx, syy, count) of the mask the
        last process() call of `stream` left on the device; k = min(count, max_boxes)."""
        boxes = np.zeros((max(max_boxes, 1), 6), np.int32)
        mom = np.zeros((max(max_boxes, 1), 4), np.int64)
        n = C.c_int32(0)
        capi.check(capi.lib().bgs_last_mask_blobs(self._h, stream, connectivity, min_w, min_h, boxes.ctypes.data_as(C.c_void_p), mom.ctypes.data_as(C.c_void_p), max_boxes, C.byref(n)))
        k = min(n.value, max_boxes)
        return boxes[:k], mom[:k], n.value

    # -- device path -----------------------------------------------------------
    @staticmethod
    def _ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def process_batch_device(self, frames, fg=None, bg=None, fg_bits=None, hip_stream=None, first=None, count=None):
        """frames/fg/bg/fg_bits: torch CUDA tensors laid out as bgs_process_batch_device documents.
        Asynchronous on hip_stream (default: torch's current stream).  Returns the out_flags."""
        import torch
        if hip_stream is None:
            hip_stream = torch.cuda.current_stream().cuda_stream
        flags = C.c_uint32(0)
        l = capi.lib()
        if first is None:
            capi.check(l.bgs_process_batch_device(self._h, self._ptr(frames), self._ptr(fg), self._ptr(bg), self._ptr(fg_bits), C.c_void_p(hip_stream), C.byref(flags)))
        else:
            capi.check(l.bgs_process_range_device(self._h, first, count, self._ptr(frames), self._ptr(fg), self._ptr(bg), self._ptr(fg_bits), C.c_void_p(hip_stream), C.byref(flags)))
        return flags.value

    def process_clip_device(self, frames, nframes, fg=None, bg=None, fg_bits=None, hip_stream=None, first=0, count=None):
        """bgs_process_clip_device: frames [nframes][count][rows][cols][ch] (torch CUDA tensors, like the outputs).  Returns the
        nframes out_flags words."""
        import torch
        if hip_stream is None:
            hip_stream = torch.cuda.current_stream().cuda_stream
        flags = (C.c_uint32 * nframes)()
        if count is None:
            count = self.n_streams - first
        capi.check(capi.lib().bgs_process_clip_device(self._h, first, count, nframes, self._ptr(frames), self._ptr(fg), self._ptr(bg), self._ptr(fg_bits),
                                                      C.c_void_p(hip_stream), flags))
        return list(flags)

    # -- introspection -----------------------------------------------------------
    def get_state(self, plane, shape, dtype, stream=0):
        out = np.empty(shape, dtype)
        n = capi.lib().bgs_get_state(self._h, stream, plane.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes)
        capi.check(n)
        assert n == out.nbytes, (n, out.nbytes)
        return out

    def frames_seen(self, stream=0):
        return capi.lib().bgs_frames_seen(self._h, stream)

    def reset_stream(self, stream):
        """bgs_reset_stream: the stream's next frame is a first frame again (model re-initialised on that call's HIP stream)."""
        capi.check(capi.lib().bgs_reset_stream(self._h, stream))

    def stream_flags(self, stream):
        f = C.c_uint32(0)
        capi.check(capi.lib().bgs_stream_flags(self._h, stream, C.byref(f)))
        return f.value

    def enable_kernel_timing(self, on=True):
        capi.check(capi.lib().bgs_enable_kernel_timing(self._h, 1 if on else 0))

    def kernel_timing(self):
        ms, n, name = C.c_double(0), C.c_int64(0), C.c_char_p()
        capi.check(capi.lib().bgs_kernel_timing(self._h, C.byref(ms), C.byref(n), C.byref(name)))
        return ms.value, n.value, (name.value or b"").decode()

    def kernel_timing_series(self, cap=16384):
        """Per-launch durations (ms) of the dominant kernel since timing was enabled."""
        buf = (C.c_float * cap)()
        n = capi.lib().bgs_kernel_timing_series(self._h, buf, cap)
        if n < 0:
            capi.check(int(n))
        return np.frombuffer(buf, dtype=np.float32, count=int(n)).copy()


def _block_methods(b):
    def set_params(self, params=None, **kw):
        self._set_block_params(b, params, kw)

    def get_params(self):
        return self._get_block_params(b)

    late = "acts from the next frame on" if b.live else "taken when the geometry is set; a later call succeeds and changes nothing"
    set_params.__doc__ = "bgs_set_%s_params (%s): %s.  Keywords change single fields of the engine's current values." % (b.name, b.classes, late)
    get_params.__doc__ = "bgs_get_%s_params (%s): the engine's current values." % (b.name, b.classes)
    for f, name in ((set_params, "set_%s_params" % b.name), (get_params, "get_%s_params" % b.name)):
        f.__name__, f.__qualname__ = name, "Engine." + name
        setattr(Engine, name, f)


# Engine.set_fuzzy_params / get_fuzzy_params, and the same for t2f, eigen, imbs and multilayer
for _b in capi.PARAM_BLOCKS:
    _block_methods(_b)


# -- stand-alone device primitives ---------------------------------------------------------------------------------
def lbsp_describe_device(img, lut, out=None, device=0, hip_stream=None):
    """img: torch CUDA uint8 [rows][cols][C] (or [rows][cols]); lut: 256 uint8 thresholds (numpy).  Returns uint16 descriptors."""
    import torch
    rows, cols = img.shape[:2]
    ch = 1 if img.dim() == 2 else img.shape[2]
    if out is None:
        out = torch.empty((rows, cols, ch), dtype=torch.int16, device=img.device)
    if hip_stream is None:
        hip_stream = torch.cuda.current_stream().cuda_stream
    lut = np.ascontiguousarray(lut, dtype=np.uint8)
    capi.check(capi.lib().bgs_lbsp_describe_device(device, C.c_void_p(img.data_ptr()), rows, cols, ch, lut.ctypes.data_as(C.c_void_p),
                                                   C.c_void_p(out.data_ptr()), C.c_void_p(hip_stream)))
    return out


def lbsp_describe_batch_device(imgs, lut, device=0, hip_stream=None):
    """imgs: torch CUDA uint8 [images][rows][cols][C]; one launch for the whole stack.  Returns int16-typed uint16 descriptors."""
    import torch
    images, rows, cols, ch = imgs.shape
    out = torch.empty((images, rows, cols, ch), dtype=torch.int16, device=imgs.device)
    if hip_stream is None:
        hip_stream = torch.cuda.current_stream().cuda_stream
    lut = np.ascontiguousarray(lut, dtype=np.uint8)
    capi.check(capi.lib().bgs_lbsp_describe_batch_device(device, C.c_void_p(imgs.data_ptr()), images, rows, cols, ch, lut.ctypes.data_as(C.c_void_p),
                                                         C.c_void_p(out.data_ptr()), C.c_void_p(hip_stream)))
    return out


MORPH_ERODE, MORPH_DILATE, MORPH_MEDIAN, MORPH_MEDIAN_BINARY, MORPH_FLOODFILL_ORIGIN = 0, 1, 2, 3, 4


def mask_morph_device(src, op, ksize=3, iterations=1, device=0, hip_stream=None):
    """src: torch CUDA uint8 [rows][cols].  op: MORPH_ERODE / MORPH_DILATE (3x3, `iterations` times) or MORPH_MEDIAN (ksize)."""
    import torch
    rows, cols = src.shape
    dst = torch.empty_like(src)
    if hip_stream is None:
        hip_stream = torch.cuda.current_stream().cuda_stream
    capi.check(capi.lib().bgs_mask_morph_device(device, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), rows, cols, op, ksize, iterations, C.c_void_p(hip_stream)))
    return dst


def canny_device(src, low, high, device=0, hip_stream=None):
    """src: torch CUDA uint8 [rows][cols] or [images][rows][cols].  cvCanny with aperture 3 and the L1 magnitude (bgs_canny_device):
    a 0 / 255 edge map of the same shape; rows * cols is at most capi.CANNY_MAX_PIXELS."""
    import torch
    images = 1 if src.dim() == 2 else src.shape[0]
    rows, cols = src.shape[-2:]
    src = src.contiguous()
    dst = torch.empty_like(src)
    if hip_stream is None:
        hip_stream = torch.cuda.current_stream().cuda_stream
    capi.check(capi.lib().bgs_canny_device(device, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), images, rows, cols, int(low), int(high), C.c_void_p(hip_stream)))
    return dst


LBPMRF_HISTOGRAM_AREA, LBPMRF_MIN_CUT_WEIGHT = 5, 8.0


def lbpmrf_mask_device(rate, rows, cols, histogram_area=LBPMRF_HISTOGRAM_AREA, min_cut_weight=LBPMRF_MIN_CUT_WEIGHT, want_labels=True, want_flow=True,
                       device=0, hip_stream=None):
    """rate: torch CUDA float32 [NH][NW] or [images][NH][NW], the background-rate map of LbpMrf's node grid for rows x cols frames
    (NH = rows - A + 1, NW = (cols - A + 1) / 2).  MotionDetection::GetMotionsMaskHU (bgs_lbpmrf_mask_device): returns (mask uint8
    [..][rows][cols] of 0 / 255, labels uint8 like rate with 1 = SINK or None, flow int32 [images] or None)."""
    import torch
    capi.check(capi.lib().bgs_lbpmrf_mask_check(rows, cols, int(histogram_area), float(min_cut_weight)))
    nh, nw = rows - histogram_area + 1, (cols - histogram_area + 1) // 2
    if rate.dtype != torch.float32 or tuple(rate.shape[-2:]) != (nh, nw) or rate.dim() not in (2, 3):
        raise ValueError("rate must be float32 [%d][%d] or [images][%d][%d]" % (nh, nw, nh, nw))
    images = 1 if rate.dim() == 2 else rate.shape[0]
    rate = rate.contiguous()
    mask = torch.empty(tuple(rate.shape[:-2]) + (rows, cols), dtype=torch.uint8, device=rate.device)
    labels = torch.empty(rate.shape, dtype=torch.uint8, device=rate.device) if want_labels else None
    flow = torch.empty(images, dtype=torch.int32, device=rate.device) if want_flow else None
    if hip_stream is None:
        hip_stream = torch.cuda.current_stream().cuda_stream
    capi.check(capi.lib().bgs_lbpmrf_mask_device(device, C.c_void_p(rate.data_ptr()), C.c_void_p(mask.data_ptr()), C.c_void_p(labels.data_ptr() if want_labels else None),
                                                 C.c_void_p(flow.data_ptr() if want_flow else None), images, rows, cols, int(histogram_area), float(min_cut_weight),
                                                 C.c_void_p(hip_stream)))
    return mask, labels, flow


def lbpmrf_mask_counters(device=0):
    """(calls of lbpmrf_mask_device on this device that did not converge - sticky, 0 when healthy -, relaxation launches of the last call); waits for the device"""
    a, b = C.c_uint64(0), C.c_uint64(0)
    capi.check(capi.lib().bgs_lbpmrf_mask_counters(device, C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def multicue_xyz(bgr, device=0, hip_stream=None):
    """bgr: torch CUDA uint8 [..., 3].  BGR2HSVxyz_Par of SJN_MultiCueBGS on every pixel (bgs_multicue_xyz_device): uint8 of the same shape."""
    import torch
    bgr = bgr.contiguous()
    out = torch.empty_like(bgr)
    if hip_stream is None:
        hip_stream = torch.cuda.current_stream().cuda_stream
    capi.check(capi.lib().bgs_multicue_xyz_device(device, C.c_void_p(bgr.data_ptr()), C.c_void_p(out.data_ptr()), bgr.numel() // 3, C.c_void_p(hip_stream)))
    return out


class MultiCueModel:
    """SJN_MultiCueBGS as a bgs_multicue handle (include/bgs_hip.h): n_streams models, each with a frame counter of its own.  Frames are torch
    CUDA uint8 [n_streams][rows][cols][3] (or [rows][cols][3] for one stream); maps come back and go in as [n_streams][rh][rw].
    process(frames) is the reference's process(), on all streams or on a range of them whatever their ages; reset_stream restarts one
    camera; process_host takes a frame in host memory; train / landmark / boxes / update are process()'s parts and need every stream at the
    same age."""

    def __init__(self, params=None, device=0, n_streams=1):
        self._h = C.c_void_p()
        self.params = params if params is not None else capi.multicue_default_params()
        self.device, self.n_streams = device, n_streams
        self.rh, self.rw = self.params.reduced_height, self.params.reduced_width
        capi.check(capi.lib().bgs_multicue_create(device, n_streams, C.byref(self.params), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            capi.lib().bgs_multicue_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _frames(self, frames):
        if frames.dim() == 3:
            frames = frames[None]
        assert frames.shape[0] == self.n_streams and frames.shape[3] == 3 and frames.dtype.itemsize == 1
        return frames.contiguous()

    @staticmethod
    def _stream(hip_stream):
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream if hip_stream is None else hip_stream)

    def train(self, frames, hip_stream=None):
        f = self._frames(frames)
        capi.check(capi.lib().bgs_multicue_train_device(self._h, C.c_void_p(f.data_ptr()), f.shape[1], f.shape[2], self._stream(hip_stream)))

    def landmark(self, frames, want_conf=True, hip_stream=None):
        """(landmark uint8 [n_streams][rh][rw] of 0 / 125 / 255, confidence float32 of the same shape or None)"""
        import torch
        f = self._frames(frames)
        lm = torch.empty((self.n_streams, self.rh, self.rw), dtype=torch.uint8, device=f.device)
        conf = torch.empty((self.n_streams, self.rh, self.rw), dtype=torch.float32, device=f.device) if want_conf else None
        capi.check(capi.lib().bgs_multicue_landmark_device(self._h, C.c_void_p(f.data_ptr()), f.shape[1], f.shape[2], C.c_void_p(lm.data_ptr()),
                                                           C.c_void_p(conf.data_ptr() if want_conf else None), self._stream(hip_stream)))
        return lm, conf

    def update(self, update_map, ghost=False, hip_stream=None):
        m = update_map if update_map.dim() == 3 else update_map[None]
        assert tuple(m.shape) == (self.n_streams, self.rh, self.rw) and m.dtype.itemsize == 1
        m = m.contiguous()
        capi.check(capi.lib().bgs_multicue_update_device(self._h, C.c_void_p(m.data_ptr()), 1 if ghost else 0, self._stream(hip_stream)))

    def boxes(self, landmark, frames, hip_stream=None):
        """The box stage (bgs_multicue_boxes_device) on landmark maps uint8 [n_streams][rh][rw] and frames.  Returns torch tensors
        (fore, ghost_map, update_map uint8 [n_streams][rh][rw], count int32 [n_streams], boxes int32 [n_streams][300][13])."""
        import torch
        f = self._frames(frames)
        lm = landmark if landmark.dim() == 3 else landmark[None]
        assert tuple(lm.shape) == (self.n_streams, self.rh, self.rw) and lm.dtype.itemsize == 1
        lm = lm.contiguous()
        fore, ghost, upd = (torch.empty((self.n_streams, self.rh, self.rw), dtype=torch.uint8, device=f.device) for _ in range(3))
        count = torch.empty(self.n_streams, dtype=torch.int32, device=f.device)
        boxes = torch.empty((self.n_streams, capi.MULTICUE_MAX_BOXES, capi.MULTICUE_BOX_FIELDS), dtype=torch.int32, device=f.device)
        capi.check(capi.lib().bgs_multicue_boxes_device(self._h, C.c_void_p(lm.data_ptr()), C.c_void_p(f.data_ptr()), f.shape[1], f.shape[2], C.c_void_p(fore.data_ptr()),
                                                        C.c_void_p(ghost.data_ptr()), C.c_void_p(upd.data_ptr()), C.c_void_p(count.data_ptr()), C.c_void_p(boxes.data_ptr()),
                                                        self._stream(hip_stream)))
        return fore, ghost, upd, count, boxes

    def process(self, frames, first=0, count=None, hip_stream=None):
        """The reference's process() on one frame per stream of [first, first + count) (bgs_multicue_process_range_device; count None: every
        stream from `first` on): the foreground image, torch uint8 [count][rows][cols]; zeros for a stream whose model trains.  The streams
        may be at different ages, and disjoint ranges may run on different HIP streams."""
        import torch
        if count is None:
            count = self.n_streams - first
        if frames.dim() == 3:
            frames = frames[None]
        assert (count < 1 or frames.shape[0] == count) and frames.shape[3] == 3 and frames.dtype.itemsize == 1  # a count below 1 is the library's to refuse
        f = frames.contiguous()
        out = torch.empty((max(count, 0), f.shape[1], f.shape[2]), dtype=torch.uint8, device=f.device)
        capi.check(capi.lib().bgs_multicue_process_range_device(self._h, first, count, C.c_void_p(f.data_ptr()), f.shape[1], f.shape[2], C.c_void_p(out.data_ptr()),
                                                                self._stream(hip_stream)))
        return out

    def reset_stream(self, stream):
        """The stream's next frame is training frame 0 (bgs_multicue_reset_stream); the other streams go on."""
        capi.check(capi.lib().bgs_multicue_reset_stream(self._h, stream))

    def frames_seen(self, stream=0):
        """The stream's g_iFrameCount: 0 before its frame 0, training_period + 2 after the last training frame."""
        return int(self.state("count", stream)[0])

    def process_host(self, frame, stream=0, channels=1):
        """process() on one frame in host memory (bgs_multicue_process), synchronous: frame is a numpy uint8 [rows][cols][3] whose rows may be
        padded (any positive row pitch, pixels contiguous within a row).  Returns numpy uint8 [rows][cols] or, channels == 3, [rows][cols][3]."""
        assert frame.ndim == 3 and frame.shape[2] == 3 and frame.dtype.itemsize == 1
        if frame.strides[2] != 1 or frame.strides[1] != 3 or frame.strides[0] <= 0:
            frame = np.ascontiguousarray(frame)
        rows, cols = frame.shape[:2]
        out = np.empty((rows, cols) if channels == 1 else (rows, cols, channels), np.uint8)
        capi.check(capi.lib().bgs_multicue_process(self._h, stream, C.c_void_p(frame.ctypes.data), rows, cols, frame.strides[0], out.ctypes.data_as(C.c_void_p),
                                                   cols * channels, channels))
        return out

    def state(self, plane, stream=0):
        """One plane of bgs_multicue_get_state as a numpy array in the reference's field order."""
        n = self.rh * self.rw
        T, TC, CS, CC = capi.MULTICUE_TEXTURE_SLOTS, capi.MULTICUE_TEXTURE_CACHE_SLOTS, capi.MULTICUE_COLOR_SLOTS, capi.MULTICUE_COLOR_CACHE_SLOTS
        shapes = {"gauss": (np.uint8, (n, 3)), "xyz": (np.uint8, (n, 3)), "conf": (np.float32, (n,)), "landmark": (np.uint8, (n,)),
                  "tbook": (np.int32, (n, 6, 2)), "tcache": (np.int32, (n, 6, 2)), "tmeans": (np.float32, (n, 6, T)), "tcache_means": (np.float32, (n, 6, TC)),
                  "tmeta": (np.int32, (n, 6, T, 3)), "tcache_meta": (np.int32, (n, 6, TC, 3)), "tref": (np.int16, (n, 6)), "tcnt": (np.int16, (n, 6)),
                  "cbook": (np.int32, (n, 2)), "ccache": (np.int32, (n, 2)), "cmeans": (np.float64, (n, CS, 3)), "ccache_means": (np.float64, (n, CC, 3)),
                  "cmeta": (np.int32, (n, CS, 3)), "ccache_meta": (np.int32, (n, CC, 3)), "cref": (np.int16, (n,)), "ccnt": (np.int16, (n,)),
                  "count": (np.int64, (1,)), "overflow": (np.int64, (1,)), "box_overflow": (np.int64, (1,))}
        dt, shape = shapes[plane]
        out = np.zeros(shape, dt)
        got = capi.check(capi.lib().bgs_multicue_get_state(self._h, stream, plane.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes))
        assert got == out.nbytes, (plane, got, out.nbytes)
        return out


BOX_FIELDS = ("x", "y", "w", "h", "area", "root")


def mask_components_device(mask, connectivity=8, max_boxes=4096, want_labels=True, device=0, hip_stream=None):
    """Connected components of a torch CUDA uint8 mask [rows][cols] (bgs_mask_components_device).
    Returns (labels int32 [rows][cols] or None, boxes int32 [min(count, max_boxes)][6] = BOX_FIELDS, count)."""
    import torch
    rows, cols = mask.shape
    if hip_stream is None:
        hip_stream = torch.cuda.current_stream().cuda_stream
    labels = torch.empty((rows, cols), dtype=torch.int32, device=mask.device) if want_labels else None
    boxes = torch.zeros((max(max_boxes, 1), 6), dtype=torch.int32, device=mask.device)
    count = torch.zeros(1, dtype=torch.int32, device=mask.device)
    work = torch.empty(capi.lib().bgs_mask_components_workspace(rows, cols), dtype=torch.uint8, device=mask.device)
    capi.check(capi.lib().bgs_mask_components_device(device, C.c_void_p(mask.data_ptr()), rows, cols, connectivity,
                                                     C.c_void_p(labels.data_ptr() if want_labels else 0), C.c_void_p(boxes.data_ptr()), max_boxes,
                                                     C.c_void_p(count.data_ptr()), C.c_void_p(work.data_ptr()), C.c_void_p(hip_stream)))
    n = int(count.item())
    return labels, boxes[:min(n, max_boxes)], n


def mask_components_batch_device(masks, connectivity=8, max_boxes=65536, want_labels=False, device=0, hip_stream=None):
    """Connected components of a stack of masks, torch CUDA uint8 [images][rows][cols], in one set of launches
    (bgs_mask_components_batch_device).  Returns (labels or None, boxes int32 [min(total, max_boxes)][6], offsets int32 [images+1]):
    image k owns boxes[offsets[k]:offsets[k+1]]."""
    import torch
    images, rows, cols = masks.shape
    if hip_stream is None:
        hip_stream = torch.cuda.current_stream().cuda_stream
    labels = torch.empty((images, rows, cols), dtype=torch.int32, device=masks.device) if want_labels else None
    boxes = torch.zeros((max(max_boxes, 1), 6), dtype=torch.int32, device=masks.device)
    offsets = torch.zeros(images + 1, dtype=torch.int32, device=masks.device)
    work = torch.empty(capi.lib().bgs_mask_components_batch_workspace(images, rows, cols), dtype=torch.uint8, device=masks.device)
    capi.check(capi.lib().bgs_mask_components_batch_device(device, C.c_void_p(masks.data_ptr()), images, rows, cols, connectivity,
                                                           C.c_void_p(labels.data_ptr() if want_labels else 0), C.c_void_p(boxes.data_ptr()), max_boxes,
                                                           C.c_void_p(offsets.data_ptr()), C.c_void_p(work.data_ptr()), C.c_void_p(hip_stream)))
    off = offsets.cpu()
    return labels, boxes[:min(int(off[-1]), max_boxes)], off


def mask_blobs_batch_device(masks, connectivity=8, max_boxes=65536, device=0, hip_stream=None):
    """bgs_mask_blobs_batch_device: boxes int32 [k][6], moments int64 [k][4] (sx, sy, sxx, syy), offsets int32 [images+1]."""
    import torch
    images, rows, cols = masks.shape
    if hip_stream is None:
        hip_stream = torch.cuda.current_stream().cuda_stream
    boxes = torch.zeros((max(max_boxes, 1), 6), dtype=torch.int32, device=masks.device)
    mom = torch.zeros((max(max_boxes, 1), 4), dtype=torch.int64, device=masks.device)
    offsets = torch.zeros(images + 1, dtype=torch.int32, device=masks.device)
    work = torch.empty(capi.lib().bgs_mask_components_batch_workspace(images, rows, cols), dtype=torch.uint8, device=masks.device)
    capi.check(capi.lib().bgs_mask_blobs_batch_device(device, C.c_void_p(masks.data_ptr()), images, rows, cols, connectivity, C.c_void_p(boxes.data_ptr()),
                                                      C.c_void_p(mom.data_ptr()), max_boxes, C.c_void_p(offsets.data_ptr()), C.c_void_p(work.data_ptr()), C.c_void_p(hip_stream)))
    off = offsets.cpu()
    k = min(int(off[-1]), max_boxes)
    return boxes[:k], mom[:k], off


# -- N3 frame preparation ------------------------------------------------------------------------------------------------
def ingest_device(cfg, frames, device=0, hip_stream=None):
    """bgs_ingest_device: frames torch CUDA uint8 [images][rows][cols][C] (or [images][rows][cols]); returns the prepared frames."""
    import torch
    images, rows, cols = frames.shape[:3]
    ch = 1 if frames.dim() == 3 else frames.shape[3]
    r, c = C.c_int(0), C.c_int(0)
    capi.check(capi.lib().bgs_ingest_size(C.byref(cfg), rows, cols, C.byref(r), C.byref(c)))
    out = torch.empty((images, r.value, c.value) if frames.dim() == 3 else (images, r.value, c.value, ch), dtype=torch.uint8, device=frames.device)
    ws = capi.lib().bgs_ingest_workspace(C.byref(cfg), images, rows, cols, ch)
    work = torch.empty(max(ws, 1), dtype=torch.uint8, device=frames.device)
    if hip_stream is None:
        hip_stream = torch.cuda.current_stream().cuda_stream
    capi.check(capi.lib().bgs_ingest_device(device, C.byref(cfg), C.c_void_p(frames.data_ptr()), images, rows, cols, ch, frames.stride(1),
                                            C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr()) if ws else None, C.c_void_p(hip_stream)))
    return out


def ingest_host(cfg, frame, device=0):
    """bgs_ingest_host: frame numpy uint8 HxW or HxWxC (any row stride); returns the prepared frame."""
    rows, cols = frame.shape[:2]
    ch = 1 if frame.ndim == 2 else frame.shape[2]
    if frame.strides[-1] != 1 or (frame.ndim == 3 and frame.strides[1] != ch):
        frame = np.ascontiguousarray(frame)
    r, c = C.c_int(0), C.c_int(0)
    capi.check(capi.lib().bgs_ingest_size(C.byref(cfg), rows, cols, C.byref(r), C.byref(c)))
    out = np.empty((r.value, c.value) if frame.ndim == 2 else (r.value, c.value, ch), np.uint8)
    capi.check(capi.lib().bgs_ingest_host(device, C.byref(cfg), frame.ctypes.data_as(C.c_void_p), rows, cols, ch, frame.strides[0],
                                          out.ctypes.data_as(C.c_void_p), out.strides[0]))
    return out


class Group:
    """bgs_group: several classes on the same frames (include/bgs_hip.h, GROUPS) - the byte-stream classes among them as one fused
    kernel, the rest as member engines.  Binding only: no arithmetic here."""

    def __init__(self, algos, params=None, device=0, n_streams=1):
        self.algos = list(algos)
        self.n_streams = n_streams
        n = len(self.algos)
        self._params = [(p if p is not None else capi.default_params(a)) for a, p in zip(self.algos, params or [None] * n)]
        arr = (C.c_int * n)(*self.algos)
        pp = (C.c_void_p * n)(*[C.cast(C.byref(p), C.c_void_p) for p in self._params])
        self._h = C.c_void_p()
        capi.check(capi.lib().bgs_group_create(arr, pp, n, device, n_streams, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            capi.lib().bgs_group_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def is_fused(self, index):
        return capi.lib().bgs_group_is_fused(self._h, index) == 1

    def set_params(self, index, params):
        capi.check(capi.lib().bgs_group_set_params(self._h, index, C.byref(params)))
        self._params[index] = params

    def set_option(self, option, value):
        capi.check(capi.lib().bgs_group_set_option(self._h, option, int(value)))

    def set_geometry(self, rows, cols, channels):
        capi.check(capi.lib().bgs_group_set_geometry(self._h, rows, cols, channels))

    def process(self, frame, want_bg=True):
        """bgs_group_process (single-stream groups): returns [(mask or None, background or None)] per class, None where the
        reference leaves the output untouched."""
        assert frame.dtype == np.uint8
        rows, cols = frame.shape[:2]
        ch = 1 if frame.ndim == 2 else frame.shape[2]
        frame = np.ascontiguousarray(frame)
        n = len(self.algos)
        fgs = [np.empty((rows, cols), np.uint8) for _ in range(n)]
        bgs_ = [np.empty((rows, cols, 1 if a == capi.ASBL else ch), np.uint8) if want_bg else None for a in self.algos]
        pf = (C.c_void_p * n)(*[f.ctypes.data for f in fgs])
        pb = (C.c_void_p * n)(*[(b.ctypes.data if b is not None else None) for b in bgs_])
        flags = (C.c_uint32 * n)()
        capi.check(capi.lib().bgs_group_process(self._h, frame.ctypes.data_as(C.c_void_p), rows, cols, ch, frame.strides[0], pf, None, pb, None, flags))
        out = []
        for i in range(n):
            f = flags[i]
            b = bgs_[i]
            if b is not None and b.shape[2] == 1:
                b = b[:, :, 0]
            out.append((fgs[i] if f & capi.FG_VALID else None, b if (b is not None and f & capi.BG_VALID) else None))
        return out

    def process_batch_device(self, frames, fgs=None, bgs_=None, hip_stream=None):
        """bgs_group_process_batch_device: frames [n_streams][rows][cols][ch] (torch CUDA tensor), fgs / bgs_: lists of tensors or None
        per class.  Asynchronous on hip_stream (default: torch's current stream).  Returns the per-class out_flags."""
        import torch
        if hip_stream is None:
            hip_stream = torch.cuda.current_stream().cuda_stream
        n = len(self.algos)
        pf = (C.c_void_p * n)(*[(t.data_ptr() if t is not None else None) for t in (fgs or [None] * n)])
        pb = (C.c_void_p * n)(*[(t.data_ptr() if t is not None else None) for t in (bgs_ or [None] * n)])
        flags = (C.c_uint32 * n)()
        capi.check(capi.lib().bgs_group_process_batch_device(self._h, C.c_void_p(frames.data_ptr()), pf, pb, C.c_void_p(hip_stream), flags))
        return list(flags)

    def get_state(self, index, plane, shape, dtype, stream=0):
        out = np.empty(shape, dtype)
        n = capi.lib().bgs_group_get_state(self._h, index, stream, plane.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes)
        capi.check(n)
        assert n == out.nbytes, (n, out.nbytes)
        return out

    def frames_seen(self):
        return capi.lib().bgs_group_frames_seen(self._h)

    def enable_kernel_timing(self, on=True):
        capi.check(capi.lib().bgs_group_enable_kernel_timing(self._h, 1 if on else 0))

    def kernel_timing(self):
        ms, n = C.c_double(0), C.c_int64(0)
        capi.check(capi.lib().bgs_group_kernel_timing(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value
