"""float32 / float64 numpy restatement of package_bgs/tb T2FGMM_UM / T2FGMM_UV (USTC_BGS types 17 and 18), written from
T2FGMM.cpp:106-303 and T2FGMM_UM.cpp:29-83, plus the cases and the reader of tests/golden/t2f_ref.npz (not a test module).

One numpy operation per rounding of the source: every array is float32, the two running sums the source keeps in double are
float64, and both qsort calls are a stable insertion by adjacent swaps (glibc's qsort keeps equal keys in order).  All pixels of a
frame advance together under boolean masks; the mode loop keeps the source's order, its shrinking count included.

The fixture comes from the reference's unmodified tb/T2FGMM.cpp + dp/Image.cpp compiled behind oracle/ref_stub;
tests/test_t2f_cpu.py holds this restatement to it bit for bit, tests/test_gpu_16_t2f.py the HIP kernels to both."""
import json
import os

import numpy as np

import dp_ref

f32, f64 = np.float32, np.float64
UM, UV = 0, 1
TYPES = ("um", "uv")
CLASS_NAMES = {"um": "T2FGMM_UM", "uv": "T2FGMM_UV"}
DEFAULTS = dict(threshold=9.0, alpha=0.01, km=1.5, kv=float(f32(0.6)), gaussians=3)  # T2FGMM_UM.cpp:19 (km / kv are float members)
FIELDS = 6  # GMM {variance, muR, muG, muB, weight, significants} (dp/GrimsonGMM.h)
VAR, MU, WEIGHT, SIG = 0, 1, 4, 5
PLANE_PIXELS = 1024  # whole-model planes are stored for the cases of at most this many pixels

TILE = "scene:15:16:64:6"     # 1 024 pixels: exactly four state tiles, npix % 64 == 0; 15 frames = one 8 + 4 + 2 + 1 clip
RAGGED = "scene:17:37:53:5"   # 1 961 pixels: no multiple of 64 or of the 256-pixel state tile; cases take 15-frame windows of it
MODES = "corners:30:8:12:8"   # 96 pixels
SMALL = "corners:20:7:11:7"   # 77 pixels: the parameter cases


def cases():
    """Ordered {case: params}: the wrapper's values + `input` (a dp_ref clip spec or frames_96x80) + optional `window`."""
    c = {}

    def add(name, inp, window=None, **kw):
        p = dict(DEFAULTS, input=inp, **kw)
        if window:
            p["window"] = list(window)
        c[name] = p

    add("default", "frames_96x80")
    add("tile", TILE)
    add("ragged", RAGGED, (0, 15))
    add("ragged_o1", RAGGED, (1, 16))  # one seeded clip entered 1 and 2 frames late: the streams of the batch test
    add("ragged_o2", RAGGED, (2, 17))
    add("tiny5x7", "scene:12:5:7:3")
    add("tiny1x1", "random:12:1:1:4")
    for K in (1, 2, 4, 5):
        add("modes_k%d" % K, MODES, gaussians=K)
    add("thr2_km3_kv03", SMALL, threshold=2.0, km=3.0, kv=float(f32(0.3)))
    add("alpha05", SMALL, alpha=0.5)
    add("ties", dp_ref.TIES, alpha=float(f32(1e-8)))
    return c


def scene_clip(T, H, W, seed):
    """A dark static background and three bright rectangles that move: both classes see matches that tighten the variance and
    jumps of about 200 in every channel.  (On uniform noise T2FGMM_UM calls nearly everything background and T2FGMM_UV nearly
    everything foreground.)  Every eighth column carries +-3 noise; the others repeat their bytes exactly, so their modes go through
    the same few float values and the stored planes deflate."""
    rng = np.random.default_rng(seed)
    base = rng.integers(20, 61, (H, W, 3)).astype(np.int16)
    out = np.empty((T, H, W, 3), np.uint8)
    bh, bw = max(1, H // 4), max(1, W // 8)
    pos = rng.integers(0, 1 << 16, (3, 2))
    col = rng.integers(200, 251, (3, 3))
    noisy = (np.arange(W) % 8 == 0)[None, :, None]
    for t in range(T):
        f = base + rng.integers(-3, 4, (H, W, 3)) * noisy
        for b in range(3):
            y0, x0 = (pos[b, 0] + t * b // 2) % H, (pos[b, 1] + t * (3 - b)) % W
            yy, xx = (np.arange(y0, y0 + bh) % H)[:, None], (np.arange(x0, x0 + bw) % W)[None, :]
            f[yy, xx] = col[b] + rng.integers(-3, 4, (bh, bw, 3)) * noisy[:, xx[0]]
        out[t] = np.clip(f, 0, 255)
    return out


def corners_clip(T, H, W, seed):
    """Every pixel dwells on one of six colours of its own for a random stretch, with +-3 noise.  The six are corners of the colour
    cube, so any two differ by about 255 in at least one channel: far enough for a new mode under either class's distance, and two
    channels apart is foreground under T2FGMM_UM's (dp_ref.modes_clip's palette is not: UM matches most of its jumps).  Noise on
    every eighth column only, as in scene_clip."""
    rng = np.random.default_rng(seed)
    corner = np.array([[(c >> b) & 1 for b in range(3)] for c in range(8)], np.int16)
    pick = np.argsort(rng.random((H, W, 8)), axis=-1)[..., :6]                     # six of the eight, per pixel
    pal = np.where(corner[pick] == 1, 250, 5) + rng.integers(-5, 6, (H, W, 6, 3))  # [H][W][6][3]
    out = np.empty((T, H, W, 3), np.uint8)
    cur = np.zeros((H, W), np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    for t in range(T):
        cur = np.where(rng.random((H, W)) < 0.4, rng.integers(0, 6, (H, W)), cur)
        out[t] = np.clip(pal[yy, xx, cur] + rng.integers(-3, 4, (H, W, 3)) * (xx % 8 == 0)[..., None], 0, 255)
    return out


def frames_of(p):
    if p["input"] == "frames_96x80":
        f = np.load(os.path.join(dp_ref.GOLDEN, "frames_96x80.npz"))["frames"]
    elif p["input"].split(":")[0] in ("scene", "corners"):
        kind, T, H, W, seed = p["input"].split(":")
        f = {"scene": scene_clip, "corners": corners_clip}[kind](int(T), int(H), int(W), int(seed))
    else:
        f = dp_ref.clip(p["input"])
    if "window" in p:
        f = f[p["window"][0]:p["window"][1]]
    return np.ascontiguousarray(f)


class T2FGMM:
    """One stream's model.  modes: [K][6][n] float32 in the source's struct order; count: [n] uint8.  `ties` counts the sort
    comparisons that met two equal keys, um_inside / um_outside what their names say."""

    def __init__(self, typ, n, threshold=9.0, alpha=0.01, km=1.5, kv=0.6, gaussians=3):
        self.typ, self.n, self.K = typ, n, int(gaussians)
        self.low = f32(threshold)           # params.LowThreshold() = threshold: double -> float
        self.high = f32(2) * self.low       # 2 * params.LowThreshold(), in float
        self.alpha = f32(alpha)
        self.km, self.kv = f32(f32(km)), f32(f32(kv))  # float members, float params, float model members
        self.modes = np.zeros((self.K, FIELDS, n), f32)  # InitModel
        self.count = np.zeros(n, np.uint8)
        self.ties = 0
        self.um_inside = self.um_outside = 0  # evaluations of each branch of the UM interval test on modes that were tried

    def _swap(self, a, b, sel):
        m = self.modes
        t = m[a][:, sel].copy()
        m[a][:, sel] = m[b][:, sel]
        m[b][:, sel] = t

    def _sort(self, nm):
        m = self.modes
        for i in range(1, self.K):
            stop = ~(i < nm)
            for j in range(i, 0, -1):
                self.ties += int(np.count_nonzero(~stop & (m[j - 1, SIG] == m[j, SIG])))
                sw = ~stop & (m[j - 1, SIG] < m[j, SIG])
                self._swap(j - 1, j, sw)
                stop |= ~sw

    def _H(self, px, mu, var, d, tr):
        if self.typ == UM:
            km = self.km
            kmv = km * var
            outside = (px < mu - kmv) | (px > mu + kmv)
            h_out = ((f32(2) * km) * d) / var
            h_in = ((d * d) / ((f32(2) * var) * var) + (km * d) / var) + (km * km) / f32(2)
            self.um_inside += int(np.count_nonzero(tr & ~outside))
            self.um_outside += int(np.count_nonzero(tr & outside))
            return np.where(outside, h_out, h_in).astype(f32)
        kv = self.kv
        c = f32(1) / (kv * kv) - kv * kv
        e = px - mu
        return ((c * e) * e) / (f32(2) * var)

    def step(self, frame):
        """T2FGMM::Subtract on one frame [H][W][3] (or [n][3]); returns the high-threshold mask [n] (0 / 255)."""
        K, n, m = self.K, self.n, self.modes
        px = np.ascontiguousarray(frame).reshape(n, 3).astype(f32)
        nm = self.count.astype(np.int64)
        alpha = self.alpha
        oma = f32(1) - alpha
        with np.errstate(all="ignore"):
            s = np.zeros(n, f64)
            bgG = np.zeros(n, np.int64)
            stop = np.zeros(n, bool)
            for k in range(K):
                act = (k < nm) & ~stop
                c = act & (s < f64(f32(0.75)))
                bgG += c
                s = np.where(c, s + m[k, WEIGHT].astype(f64), s)
                stop |= act & ~c
            fits = np.zeros(n, bool)
            bg_high = np.zeros(n, bool)
            total = np.zeros(n, f32)
            for k in range(K):
                act = k < nm
                weight = m[k, WEIGHT].copy()
                var = m[k, VAR].copy()
                tr = act & ~fits
                d = [np.abs(m[k, MU + ch] - px[:, ch]) for ch in range(3)]
                H = [self._H(px[:, ch], m[k, MU + ch], var, d[ch], tr) for ch in range(3)]
                dist = (H[0] * H[0] + H[1] * H[1]) + H[2] * H[2]
                bg_high |= tr & (dist < self.high * var) & (k < bgG)
                match = tr & (dist < self.low * var)
                kk = alpha / weight
                w_m = oma * weight + alpha
                sn = var + kk * (dist - var)
                v_m = np.where(sn < 4, f32(4), np.where(sn > 180, f32(180), sn)).astype(f32)
                for ch in range(3):
                    m[k, MU + ch] = np.where(match, m[k, MU + ch] - kk * d[ch], m[k, MU + ch])
                m[k, VAR] = np.where(match, v_m, var)
                w_d = oma * weight
                neg = act & ~match & (w_d < 0.0)
                w_d = np.where(neg, f32(0), w_d)
                nm = nm - neg
                w_new = np.where(match, w_m, np.where(act, w_d, weight)).astype(f32)
                m[k, WEIGHT] = w_new
                m[k, SIG] = np.where(act, w_new / np.sqrt(m[k, VAR]), m[k, SIG])
                total = np.where(act, total + w_new, total)
                fits |= match
            inv = (f64(1.0) / total.astype(f64)).astype(f32)
            for k in range(K):
                act = k < nm
                m[k, WEIGHT] = np.where(act, m[k, WEIGHT] * inv, m[k, WEIGHT])
                m[k, SIG] = np.where(act, m[k, WEIGHT] / np.sqrt(m[k, VAR]), m[k, SIG])
            self._sort(nm)
            nofit = ~fits
            nm = np.where(nofit & (nm < K), nm + 1, nm)
            last = nm - 1
            for k in range(K):
                sel = nofit & (last == k)
                for ch in range(3):
                    m[k, MU + ch] = np.where(sel, px[:, ch], m[k, MU + ch])
                m[k, VAR] = np.where(sel, f32(36), m[k, VAR])
                m[k, SIG] = np.where(sel, f32(0), m[k, SIG])
                m[k, WEIGHT] = np.where(sel, np.where(nm == 1, f32(1), alpha), m[k, WEIGHT])
            sm = np.zeros(n, f32)
            for k in range(K):
                sm = np.where(nofit & (k < nm), sm + m[k, WEIGHT], sm)
            inv2 = (f64(1.0) / sm.astype(f64)).astype(f32)
            for k in range(K):
                act = nofit & (k < nm)
                m[k, WEIGHT] = np.where(act, m[k, WEIGHT] * inv2, m[k, WEIGHT])
                m[k, SIG] = np.where(act, m[k, WEIGHT] / np.sqrt(m[k, VAR]), m[k, SIG])
            self._sort(nm)
        self.count = nm.astype(np.uint8)
        return np.where(bg_high, 0, 255).astype(np.uint8)

    def planes(self):
        """"modes" as bgs_get_state hands it out: [K*6][n]."""
        return self.modes.reshape(self.K * FIELDS, self.n).copy()


def model_of(typ, p, n):
    return T2FGMM(TYPES.index(typ), n, p["threshold"], p["alpha"], p["km"], p["kv"], p["gaussians"])


def run(typ, p, frames):
    """masks [T][H][W], the model after the last frame."""
    T, H, W = frames.shape[:3]
    mdl = model_of(typ, p, H * W)
    masks = np.array([mdl.step(f).reshape(H, W) for f in frames])
    return masks, mdl


def below_count(modes, count, K):
    """[K][6][n] bool: the floats of the modes below each pixel's count (the only ones the source defines)."""
    return np.broadcast_to((np.arange(K)[:, None, None] < count[None, None, :]), (K, FIELDS, count.size))


_loaded = None


def load():
    """{(type, case): record}: params, frames (CRC-checked), masks [T][H][W], and for small cases modes [K*6][n] / nmodes [n]."""
    global _loaded
    if _loaded is None:
        z = np.load(os.path.join(dp_ref.GOLDEN, "t2f_ref.npz"))
        out = {}
        for typ in TYPES:
            for case in json.loads(str(z["cases"])):
                pre = "%s/%s/" % (typ, case)
                r = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
                p = json.loads(str(r["params"]))
                frames = frames_of(p)
                assert dp_ref.crc(frames) == int(r["input_crc32"]), "%s%s: the input clip differs from the one the fixture was made from" % (pre, case)
                T, H, W = (int(v) for v in r["shape"])
                masks = np.unpackbits(r["masks"], axis=-1)[..., :W].reshape(T, H, W) * np.uint8(255)
                rec = dict(params=p, frames=frames, masks=masks)
                if "modes" in r:
                    # stored as four planes of bytes (byte b of every float together): deflates far better than the words
                    rec["modes"] = np.ascontiguousarray(np.moveaxis(r["modes"], 0, -1)).view(f32).reshape(p["gaussians"] * FIELDS, H * W)
                    rec["nmodes"] = r["nmodes"]
                for a in rec.values():
                    if isinstance(a, np.ndarray):
                        a.setflags(write=False)
                out[typ, case] = rec
        _loaded = (out, json.loads(str(z["environment"])))
    return _loaded[0]


def environment():
    load()
    return _loaded[1]
