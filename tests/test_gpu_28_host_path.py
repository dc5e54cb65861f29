"""The entry points that take a frame in host memory and hand results back to host memory - bgs_process, bgs_submit / bgs_wait,
bgs_group_process, bgs_ingest_host - through the one staging lane they share (tracking_amd/csrc/host_path.h).  Frames of
67 rows go up in eight uneven bands, frames of 37 rows in one.  Every array with padded rows carries 0xA5 in the padding, which must
come back untouched; every mask, background and flag word equals the oracle's, or - VuMeter, the group's classes - what a fresh
engine computes for the same frames on another path.  bgs_multicue_process is covered by test_gpu_27_multicue_class.py."""
import ctypes as C
import functools
import mmap

import numpy as np
import pytest

from oracle import pyoracle
from tools import synth
from tracking_amd import Engine, capi
from tracking_amd.engine import Group, ingest_device

from gpu_helpers import ALGOS, _torch

pytestmark = pytest.mark.gpu

COLS, T, PAD = 53, 6, 0xA5
SHAPES = [67, 37]  # rows: eight uneven bands (67 >= 64, not a multiple of 8) and one band
CLASSES = ["FrameDifferenceBGS", "MixtureOfGaussianV2BGS", "VuMeter"]  # upload into the ring slot; banded download; gray background of colour frames
ALGO = dict(ALGOS, VuMeter=capi.VUMETER)


@functools.lru_cache(maxsize=None)
def clip(rows):
    frames = synth.random_frames(T, rows, COLS, 3, seed=rows)
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def expected(name, rows):
    """[(mask or None, background or None)] of the clip: the oracle's, or for VuMeter (no oracle class) a fresh engine's device path"""
    frames = clip(rows)
    if name != "VuMeter":
        orc = pyoracle.Oracle(ALGO[name])
        return [orc.process(f) for f in frames]
    torch = _torch()
    out = []
    with Engine(capi.VUMETER) as eng:
        eng.set_geometry(rows, COLS, 3)
        for f in frames:
            d_fg = torch.zeros((1, rows, COLS), dtype=torch.uint8, device="cuda")
            d_bg = torch.zeros((1, rows, COLS), dtype=torch.uint8, device="cuda")
            fl = eng.process_batch_device(torch.from_numpy(f.copy()).cuda().unsqueeze(0), d_fg, d_bg, None)
            torch.cuda.synchronize()
            out.append((d_fg.cpu().numpy()[0] if fl & capi.FG_VALID else None, d_bg.cpu().numpy()[0] if fl & capi.BG_VALID else None))
    return out


def bg_channels(name):
    return 1 if name == "VuMeter" else 3


def padded(rows, cols, ch, extra):
    """(whole buffer filled with 0xA5, the rows x cols x ch image inside it): each row is followed by `extra` pixels of padding"""
    buf = np.full((rows, cols + extra, ch) if ch > 1 else (rows, cols + extra), PAD, np.uint8)
    return buf, buf[:, :cols]


def page_locked_candidate(shape):
    """a contiguous array on pages of its own (hipHostRegister works on whole pages; two small malloc'd arrays may share one)"""
    n = int(np.prod(shape))
    return np.frombuffer(mmap.mmap(-1, (n + 4095) // 4096 * 4096), np.uint8, n).reshape(shape)


def check_frame(where, flags, fg, bg, want, fg_buf=None, bg_buf=None):
    wfg, wbg = want
    assert bool(flags & capi.FG_VALID) == (wfg is not None) and bool(flags & capi.BG_VALID) == (wbg is not None), (where, flags)
    assert np.array_equal(fg, wfg) if wfg is not None else (fg == PAD).all(), (where, "mask")
    if bg is not None:
        assert np.array_equal(bg.reshape(wbg.shape), wbg) if wbg is not None else (bg == PAD).all(), (where, "background")
    for buf in (fg_buf, bg_buf):
        if buf is not None:
            assert (buf[:, COLS:] == PAD).all(), (where, "padding overwritten")


def run_one(eng, mode, frame, fg, bg):
    if mode == "process":
        return eng.process_into(frame, fg, bg)
    eng.submit(frame, fg, bg)
    return eng.wait()


@pytest.mark.parametrize("mode", ["process", "submit"])
@pytest.mark.parametrize("rows", SHAPES)
@pytest.mark.parametrize("name", CLASSES)
def test_padded_rows_in_and_out(name, rows, mode):
    want = expected(name, rows)
    in_buf, frame = padded(rows, COLS, 3, 5)
    fg_buf, fg = padded(rows, COLS, 1, 7)
    bg_buf, bg = padded(rows, COLS, bg_channels(name), 3)
    with Engine(ALGO[name]) as eng:
        for t, f in enumerate(clip(rows)):
            frame[...] = f
            fg_buf[...] = PAD
            bg_buf[...] = PAD
            flags = run_one(eng, mode, frame, fg, bg)
            check_frame((name, rows, mode, t), flags, fg, bg, want[t], fg_buf, bg_buf)
            assert (in_buf[:, COLS:] == PAD).all() and np.array_equal(frame, f), "the input image was written to"


@pytest.mark.parametrize("mode", ["process", "submit"])
@pytest.mark.parametrize("rows", SHAPES)
@pytest.mark.parametrize("name", CLASSES)
def test_registered_caller_buffers(name, rows, mode):
    """BGS_OPT_HOST_REGISTER = 7 with contiguous buffers that stay allocated until the engine is closed: same results, and a role is
    page-locked from the second call on in which its image crossed the bus (an invalid output is not copied, so it is no candidate)."""
    want = expected(name, rows)
    frame = page_locked_candidate((rows, COLS, 3))
    fg = page_locked_candidate((rows, COLS))
    bg = page_locked_candidate((rows, COLS, bg_channels(name)) if bg_channels(name) > 1 else (rows, COLS))
    used = [0, 0, 0]
    with Engine(ALGO[name]) as eng:
        eng.set_option(capi.OPT_HOST_REGISTER, 7)
        for t, f in enumerate(clip(rows)):
            frame[...] = f
            fg[...] = PAD
            bg[...] = PAD
            flags = run_one(eng, mode, frame, fg, bg)
            check_frame((name, rows, mode, t), flags, fg, bg, want[t])
            used = [used[0] + 1, used[1] + (want[t][0] is not None), used[2] + (want[t][1] is not None)]
            d = eng.get_state("hostpath", (15,), np.float64)
            assert list(d[0:3]) == [float(u >= 2) for u in used], (name, t, list(d[0:6]))
            assert list(d[3:6]) == [0.0, 0.0, 0.0], (name, t, "a registration was refused")
        assert used[0] == T and (name == "FrameDifferenceBGS" or used == [T, T, T])


@pytest.mark.parametrize("rows", SHAPES)
def test_process_on_a_stream_with_a_pending_submit(rows):
    """bgs_process collects (and drops the flags of) the stream's submission in flight, then runs: the frames count on as if both
    calls had been synchronous, and a bgs_wait afterwards finds nothing pending."""
    name = "MixtureOfGaussianV2BGS"
    want = expected(name, rows)
    frames = clip(rows)
    with Engine(ALGO[name]) as eng:
        for t in range(0, T, 2):
            s_fg_buf, s_fg = padded(rows, COLS, 1, 7)
            s_bg_buf, s_bg = padded(rows, COLS, 3, 3)
            submitted = np.ascontiguousarray(frames[t])
            eng.submit(submitted, s_fg, s_bg)
            fg_buf, fg = padded(rows, COLS, 1, 2)
            bg_buf, bg = padded(rows, COLS, 3, 1)
            flags = eng.process_into(np.ascontiguousarray(frames[t + 1]), fg, bg)
            check_frame((rows, t + 1, "process"), flags, fg, bg, want[t + 1], fg_buf, bg_buf)
            # the submission's images were written when it was collected; only its flag word is dropped
            s_flags = (capi.FG_VALID if want[t][0] is not None else 0) | (capi.BG_VALID if want[t][1] is not None else 0)
            check_frame((rows, t, "collected submission"), s_flags, s_fg, s_bg, want[t], s_fg_buf, s_bg_buf)
            assert eng.wait() == 0
            assert eng.frames_seen() == t + 2


@pytest.mark.parametrize("kw", [dict(flip=1, roi_x0=3, roi_y0=5, roi_x1=43, roi_y1=36), dict(flip=1, roi_x0=2, roi_y0=1, roi_x1=50, roi_y1=66),
                                dict(roi_x0=2, roi_y0=1, roi_x1=50, roi_y1=66), dict(flip=1)])
@pytest.mark.parametrize("name", ["MixtureOfGaussianV2BGS", "FrameDifferenceBGS"])
def test_flip_and_roi_ride_on_the_upload_of_padded_rows(name, kw):
    """bgs_set_ingest with flip / ROI only: no device preparation, the staging copy reads the mapped source rows of the padded raw
    frame (31 prepared rows: one band; 65 and 67: eight)."""
    cfg = capi.default_ingest(**kw)
    in_buf, frame = padded(67, COLS, 3, 5)
    orc = pyoracle.Oracle(ALGO[name])
    with Engine(ALGO[name]) as eng:
        eng.set_ingest(cfg)
        for t, f in enumerate(clip(67)):
            frame[...] = f
            fg, bg = eng.process(frame)
            ofg, obg = orc.process(pyoracle.ingest(cfg, f))
            assert (fg is None) == (ofg is None) and (bg is None) == (obg is None), (kw, t)
            assert ofg is None or np.array_equal(fg, ofg), (kw, t)
            assert obg is None or np.array_equal(bg, obg), (kw, t)
        assert (in_buf[:, COLS:] == PAD).all()


def test_group_process_with_padded_steps():
    """bgs_group_process through raw ctypes with explicit fg_step / bg_step: every class equals its own single engine."""
    rows = 37
    names = ["FrameDifferenceBGS", "WeightedMovingVarianceBGS", "AdaptiveBackgroundLearning", "MixtureOfGaussianV2BGS"]
    algos = [ALGOS[n] for n in names]
    K = len(algos)
    singles = [Engine(a) for a in algos]
    grp = Group(algos)
    in_buf, frame = padded(rows, COLS, 3, 5)
    fgs = [padded(rows, COLS, 1, 3 + i) for i in range(K)]
    bgs_ = [padded(rows, COLS, 3, 1 + i) for i in range(K)]
    pf = (C.c_void_p * K)(*[v.ctypes.data for _, v in fgs])
    pb = (C.c_void_p * K)(*[v.ctypes.data for _, v in bgs_])
    sf = (C.c_size_t * K)(*[v.strides[0] for _, v in fgs])
    sb = (C.c_size_t * K)(*[v.strides[0] for _, v in bgs_])
    for t, f in enumerate(clip(rows)):
        frame[...] = f
        for buf, _ in fgs + bgs_:
            buf[...] = PAD
        flags = (C.c_uint32 * K)()
        capi.check(capi.lib().bgs_group_process(grp._h, frame.ctypes.data_as(C.c_void_p), rows, COLS, 3, frame.strides[0], pf, sf, pb, sb, flags))
        for i in range(K):
            check_frame((names[i], t), flags[i], fgs[i][1], bgs_[i][1], singles[i].process(f), fgs[i][0], bgs_[i][0])
    grp.close()
    for e in singles:
        e.close()


@pytest.mark.parametrize("kw", [dict(), dict(resize_percent=75, flip=1, gaussian_blur=1), dict(flip=1, roi_x0=3, roi_y0=5, roi_x1=43, roi_y1=36)])
def test_ingest_host_with_padded_source_and_destination(kw):
    torch = _torch()
    cfg = capi.default_ingest(**kw)
    f = clip(67)[0]
    want = ingest_device(cfg, torch.from_numpy(f.copy()).cuda().unsqueeze(0)).cpu().numpy()[0]
    in_buf, frame = padded(67, COLS, 3, 5)
    frame[...] = f
    out_buf = np.full((want.shape[0], want.shape[1] + 4, 3), PAD, np.uint8)
    out = out_buf[:, :want.shape[1]]
    capi.check(capi.lib().bgs_ingest_host(0, C.byref(cfg), frame.ctypes.data_as(C.c_void_p), 67, COLS, 3, frame.strides[0], out.ctypes.data_as(C.c_void_p), out.strides[0]))
    assert np.array_equal(out, want), kw
    assert (out_buf[:, want.shape[1]:] == PAD).all() and (in_buf[:, COLS:] == PAD).all()
