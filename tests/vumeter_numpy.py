"""numpy restatement of the reference's package_bgs/av/VuMeter (USTC_BGS type 31): the wrapper VuMeter::process and the model
TBackgroundVuMeter::UpdateBackground - the CPU yardstick of BGS_VUMETER (not a test module).

float32 where the reference is float, float64 where it is double.  numpy's elementwise * and + on float32 arrays are IEEE single
operations, one rounding each, nothing fused, and denormals are kept.  tests/golden/vumeter_ref.npz (outputs of the reference's
own model code) pins the model; the wrapper's gray conversion, erode and median are recalled OpenCV arithmetic.

The quirks the restatement keeps:
  * the bin of a byte is byte / binSize, and an index >= binCount (= 256 / binSize) maps to bin 0;
  * cvConvertScale on a 32F image works in float: h = fl32(h * (float)alpha), not the double product rounded once;
  * the increment is (float)(1.0 - alpha): subtracted in double, rounded once;
  * the mask compares the float bin value, promoted to double, with the double threshold;
  * the background byte is replaced when its bin is below the frame's bin AFTER the increment;
  * the mask of the first four frames is zeroed, before the post-filter;
  * SetBinSize / SetAlpha / SetThreshold replace out-of-range values and run once, on the first frame; enableFilter is live.
"""
import zlib

import numpy as np

DEFAULTS = dict(bin_size=8, alpha=0.995, threshold=0.03, enable_filter=1)  # VuMeter.cpp:19
QUIET_FRAMES = 4  # m_nCount < 5: masks of frames 1..4 are zero


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def gray_rgb(frame):
    """cvCvtColor(frame, gray, CV_RGB2GRAY) of a BGR frame: byte 0 gets the R weight (OpenCV 2.4's 14-bit fixed point)."""
    f = frame.astype(np.int32)
    return ((f[..., 0] * 4899 + f[..., 1] * 9617 + f[..., 2] * 1868 + 8192) >> 14).astype(np.uint8)


def setters(bin_size, alpha, threshold):
    """TBackgroundVuMeter::SetBinSize / SetAlpha / SetThreshold (TBackgroundVuMeter.h:47-54)."""
    return (bin_size if 0 < bin_size < 255 else 8, alpha if 0.0 < alpha < 1.0 else 0.995, threshold if 0.0 < threshold < 1.0 else 0.03)


class Model:
    """TBackgroundVuMeter behind gray frames: update(gray, background) -> raw mask; `background` is updated in place."""

    def __init__(self, bin_size=8, alpha=0.995, threshold=0.03):
        self.bin_size, self.alpha, self.threshold = setters(int(bin_size), float(alpha), float(threshold))
        self.bin_count = 256 // self.bin_size
        self.hist = None
        self.count = 0
        self.replaced = 0       # background bytes replaced so far
        self.denormal_seen = 0  # (bin, pixel) values that were f32 denormals after a frame's decay, summed over frames

    def bins(self, img):
        i = img.astype(np.int32) // self.bin_size
        return np.where(i >= self.bin_count, 0, i)

    def update(self, gray, background):
        if self.hist is None:  # Init() + Reset(): every bin exactly 0
            self.hist = np.zeros((self.bin_count,) + gray.shape, np.float32)
            self.count = 0
        self.count += 1
        self.hist *= np.float32(self.alpha)  # cvConvertScale(h, h, alpha, 0): float working type
        tiny = np.finfo(np.float32).tiny
        self.denormal_seen += int(((self.hist > 0) & (self.hist < tiny)).sum())
        rr, cc = np.indices(gray.shape)
        i = self.bins(gray)
        self.hist[i, rr, cc] += np.float32(1.0 - self.alpha)
        hi = self.hist[i, rr, cc]
        mask = np.where(hi.astype(np.float64) < self.threshold, 255, 0).astype(np.uint8)
        hj = self.hist[self.bins(background), rr, cc]
        take = hj < hi
        self.replaced += int((take & (background != gray)).sum())
        background[take] = gray[take]
        if self.count < 5:
            mask[:] = 0
        return mask


class VuMeter:
    """VuMeter::process: (mask, background) of one BGR frame, both 8UC1, from frame 1."""

    def __init__(self, bin_size=8, alpha=0.995, threshold=0.03, enable_filter=1):
        self.model = Model(bin_size, alpha, threshold)
        self.enable_filter = enable_filter
        self.background = None

    def process_gray(self, gray):
        from oracle import pyoracle
        if self.background is None:
            self.background = gray.copy()
        mask = self.model.update(gray, self.background)
        if self.enable_filter:
            mask = pyoracle.median_blur(pyoracle.erode3x3(mask), 5)
        return mask, self.background.copy()

    def process(self, frame):
        if frame.ndim != 3 or frame.shape[2] != 3:
            raise ValueError("cvCvtColor(CV_RGB2GRAY) asserts on 1-channel frames")
        return self.process_gray(gray_rgb(frame))


# ---- seeded gray clips of the fixtures ([T][H][W] uint8) ------------------------------------------------------------------------------

def box(T, H, W, seed):
    """A textured static scene with +-3 sensor noise, saturated patches (bytes 255 and >= 200) and a bright box that crosses it, so
    pixels leave their bin, come back, and backgrounds are replaced."""
    rng = np.random.RandomState(seed)
    base = rng.randint(10, 246, size=(H, W)).astype(np.int32)
    base[: H // 4, : W // 4] = 255
    base[H // 2:, : W // 5] = 205
    out = np.empty((T, H, W), np.uint8)
    bh, bw = max(H // 3, 1), max(W // 4, 1)
    for t in range(T):
        f = np.clip(base + rng.randint(-3, 4, size=(H, W)), 0, 255)
        x = (t * 2) % (W + bw) - bw
        y = (t // 3) % max(H - bh + 1, 1)
        f[y:y + bh, max(x, 0):max(x + bw, 0)] = 250 if (t // 40) % 2 == 0 else 30
        out[t] = f
    if T > 60:  # the scene itself changes half-way: the old background bins lose against the new ones
        out[T // 2:, H // 3: 2 * H // 3, W // 2:] = np.clip(out[T // 2:, H // 3: 2 * H // 3, W // 2:].astype(np.int32) // 2 + 100, 0, 255)
    return out


def leave(T, H, W, seed):
    """Every pixel spends its first three frames in one bin, then moves to another (at least two bins away) and never returns."""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 100, size=(H, W))
    b = a + rng.randint(40, 150, size=(H, W))
    out = np.empty((T, H, W), np.uint8)
    out[:3] = a
    out[3:] = b
    return out


def bgr(T, H, W, seed):
    """[T][H][W][3] colour frames: three `box` clips with their own textures and noise as B, G, R (the boxes move together)."""
    return np.stack([box(T, H, W, seed * 3 + k) for k in range(3)], axis=-1)


def clip(name):
    """Gray frames of a fixture input: 'gray:frames_96x80' (RGB2GRAY of the committed clip) or '<generator>:T:H:W:seed'."""
    import os
    if name == "gray:frames_96x80":
        return gray_rgb(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames_96x80.npz"))["frames"])
    kind, T, H, W, seed = name.split(":")
    return {"box": box, "leave": leave}[kind](int(T), int(H), int(W), int(seed))
