"""float64 numpy restatement of package_bgs/dp DPEigenbackgroundBGS (USTC_BGS type 15), written from Eigenbackground.cpp:76-190 and
DPEigenbackgroundBGS.cpp:29-82, plus the seeded clips, the cases and the reader of tests/golden/eigen_ref.npz (not a test module).

The reference's PCA is OpenCV's cvCalcPCA, which cannot be rebuilt here and runs in float32: what is pinned bit for bit is everything
around it (the history / build / detect schedule, the per-channel distance, the float thresholds, embeddedDim rows, float `proj` and
float `result`); the PCA itself is pinned as mathematics, within a measured tolerance.  The fixture comes from the
reference's unmodified dp/Eigenbackground.cpp + dp/Image.cpp behind a stand-in header whose three PCA calls are written in double and
round into the CV_32F matrices the model allocates.

TOL_FLOOR is the largest |result| difference between this restatement in float64 and its own float-storage variant (avg, eigenvectors,
coefficients and result rounded to float32, as the reference stores them) over all fixture cases: tests/test_eigen_cpu.py measures
it and holds it below the constant here.  The engine sums in another order and its Jacobi is not LAPACK's: TOL_RESULT = 8 x TOL_FLOOR
is headroom for a handful of ulps at 255, not for a wrong subspace, which shows as errors of whole grey levels.  A pixel of a frame is
near-threshold iff for some channel | |x - r64| - sqrt(thr) | <= 4 TOL_RESULT for thr in {low, high}; masks are compared outside
that band only, and the band may hold at most BAND_SHARE of a case's pixel-frames."""
import json
import os
import zlib

import numpy as np

f32, f64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLASS_NAME = "DPEigenbackground"
DEFAULTS = dict(threshold=225, history_size=20, embedded_dim=10)  # DPEigenbackgroundBGS.cpp:19
PLANE_PIXELS = 1024   # avg, eigenvalues and the last result are stored for the cases of at most this many pixels
TOL_FLOOR = 1.7e-5    # measured by tests/test_eigen_cpu.py (it prints the figure): 1.65e-5, about 1 ulp at 255
TOL_RESULT = 8 * TOL_FLOOR
BAND_SHARE = 0.005
EIGENGAP = 1.25       # lambda_M / lambda_{M+1} of every case that claims parity
NO_PARITY = ("tiny1x1",)  # rank below M: the reference's result there depends on normalised rounding residue


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xffffffff


def cases():
    """Ordered {case: params}: the wrapper's three values + `input` = "kind:T:H:W:seed" + optional `window` and `box`."""
    c = {}

    def add(name, inp, window=None, **kw):
        p = dict(DEFAULTS, input=inp, **kw)
        if window:
            p["window"] = list(window)
        c[name] = p

    add("default", "pca:30:24:32:1")
    add("tile", "pca:28:16:64:2")
    add("ragged", "pca:30:37:53:3", (0, 28))
    add("ragged_o1", "pca:30:37:53:3", (1, 29))  # one seeded clip entered 1 and 2 frames late: the streams of the batch test
    add("ragged_o2", "pca:30:37:53:3", (2, 30))
    add("chunks", "pca:8:75:77:4", history_size=4, embedded_dim=2)  # 3 n = 17 325 elements: three projection chunks, the last one ragged
    add("tiny3x3", "pca:24:3:3:5")
    add("h8_m3", "pca:14:9:13:6", history_size=8, embedded_dim=3)
    add("h32_m31", "pca:38:9:13:7", history_size=32, embedded_dim=31)
    add("h2_m1", "pca:6:9:13:8", history_size=2, embedded_dim=1)
    add("thr0", "pca:24:5:7:19", threshold=0)
    add("thr100", "pca:26:9:13:10", threshold=100)
    add("static", "static:24:9:13:11")
    add("tiny1x1", "pca:24:1:1:12")
    return c


def pca_clip(T, H, W, seed, quiet):
    """base + sum_k a_k(t) pattern_k + noise: 12 fixed random patterns, amplitudes 40 x 0.75^k, +-1 noise, so the top subspaces are
    well conditioned (no two PCA implementations agree on an ill-conditioned one).  Frames from `quiet` on add a moving bright box."""
    rng = np.random.default_rng(seed)
    base = rng.integers(60, 180, (H, W, 3)).astype(f64)
    pat = rng.uniform(-1, 1, (12, H, W, 3))
    amp = 40 * 0.75 ** np.arange(12)
    out = np.empty((T, H, W, 3), np.uint8)
    bh, bw = max(1, H // 3), max(1, W // 3)
    if H * W <= 35:
        bh, bw = max(1, H // 2), max(1, W // 4)
    elif H * W <= 200:
        bh, bw = (H + 1) // 2, (W + 1) // 2  # at least 20 foreground and 20 background pixels from 36 pixels up
    y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
    for t in range(T):
        a = amp * rng.uniform(-1, 1, 12)
        f = base + np.tensordot(a, pat, 1) + rng.integers(-1, 2, (H, W, 3))
        if t >= quiet:
            yy, xx = (np.arange(y0 + t, y0 + t + bh) % H)[:, None], (np.arange(x0 + 2 * t, x0 + 2 * t + bw) % W)[None, :]
            f[yy, xx] += 90
        out[t] = np.clip(np.rint(f), 0, 255)
    return out


def static_clip(T, H, W, seed, quiet):
    """All history frames identical: the centred Gram matrix is exactly 0, every eigenvector row is zero and result = avg = the bytes."""
    rng = np.random.default_rng(seed)
    one = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    out = np.repeat(one[None], T, 0)
    for t in range(quiet, T):
        rows = [(t * 2) % H, (t * 2 + 1) % H]
        out[t, rows] = 255 - one[rows]
    return out


def frames_of(p):
    kind, T, H, W, seed = p["input"].split(":")
    quiet = p["history_size"] + 2  # the box stays out of every window's history
    f = {"pca": pca_clip, "static": static_clip}[kind](int(T), int(H), int(W), int(seed), quiet)
    if "window" in p:
        f = f[p["window"][0]:p["window"][1]]
    return np.ascontiguousarray(f)


def thresholds(p):
    low = f32(p["threshold"])  # params.LowThreshold() = threshold: int -> float
    return low, f32(2) * low   # 2 * params.LowThreshold(), in float


class Eigenbackground:
    """One stream's model.  storage = f64: the mathematics; f32: avg, eigenvectors, coefficients and result rounded to float32."""

    def __init__(self, p, n, storage=f64):
        self.H, self.M, self.n, self.st = int(p["history_size"]), int(p["embedded_dim"]), n, storage
        self.low, self.high = thresholds(p)
        self.history = np.zeros((self.H, n * 3), np.uint8)
        self.t = 0
        self.avg = self.lam = self.E = self.coeff = self.result = None

    def build(self):
        H, X = self.H, self.history.astype(np.int64)
        G = X @ X.T                                            # exact
        r = G.sum(1)
        A = H * H * G - H * (r[:, None] + r[None, :]) + G.sum()  # exact: H^2 x the centred Gram matrix
        lam, V = np.linalg.eigh(A.astype(f64) / f64(H * H))
        order = np.argsort(-lam, kind="stable")
        lam, V = lam[order], V[:, order]
        S = X.sum(0)
        Xc = X.astype(f64) - S.astype(f64) / H
        W = np.zeros((self.M, H))
        for i in range(self.M):
            if not lam[i] <= H * 2.0 ** -40 * lam[0]:          # the zero-row rule: what cv::normalize makes of a zero vector
                W[i] = V[:, i] / np.sqrt(lam[i])
        self.lam = lam
        self.E = (W @ Xc).astype(self.st)
        self.avg = (S.astype(f32) / f32(H)) if self.st is f32 else S.astype(f64) / H

    def step(self, frame):
        x = frame.reshape(-1)
        if self.t < self.H:
            self.history[self.t] = x
            self.t += 1
            return np.zeros(self.n, np.uint8)
        if self.t == self.H:
            self.build()
        xd = x.astype(f64)
        self.coeff = (self.E.astype(f64) @ (xd - self.avg.astype(f64))).astype(self.st)
        self.result = (self.avg.astype(f64) + self.coeff.astype(f64) @ self.E.astype(f64)).astype(self.st)
        dist = (xd - self.result.astype(f64)) ** 2
        self.t += 1
        return np.where((dist > f64(self.high)).reshape(self.n, 3).any(1), 255, 0).astype(np.uint8)


def run(p, frames, storage=f64):
    """masks [T][H][W], results [T - Hs][3n] of the detecting frames, the model after the last frame."""
    T, H, W = frames.shape[:3]
    mdl = Eigenbackground(p, H * W, storage)
    masks, results = [], []
    for f in frames:
        masks.append(mdl.step(f).reshape(H, W))
        if mdl.result is not None:
            results.append(mdl.result.copy())
    return np.array(masks), np.array(results), mdl


def band(p, frame, r64):
    """[n] bool: the pixels of `frame` that are near a threshold, given the float64 reconstruction."""
    d = np.abs(frame.reshape(-1).astype(f64) - r64)
    near = np.zeros(d.shape, bool)
    for thr in thresholds(p):
        near |= np.abs(d - np.sqrt(f64(thr))) <= 4 * TOL_RESULT
    return near.reshape(-1, 3).any(1)


_loaded = None


def load():
    """{case: record}: params, frames (CRC-checked), masks [T][H][W], and for small cases avg f32 [3n], eigenvalues f64 [Hs],
    result f32 [3n] (the last frame's)."""
    global _loaded
    if _loaded is None:
        z = np.load(os.path.join(GOLDEN, "eigen_ref.npz"))
        out = {}
        for case in json.loads(str(z["cases"])):
            pre = case + "/"
            r = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
            p = json.loads(str(r["params"]))
            frames = frames_of(p)
            assert crc(frames) == int(r["input_crc32"]), "%s: the input clip differs from the one the fixture was made from" % case
            T, H, W = (int(v) for v in r["shape"])
            rec = dict(params=p, frames=frames, masks=np.unpackbits(r["masks"], axis=-1)[..., :W].reshape(T, H, W) * np.uint8(255))
            if "avg" in r:
                rec["avg"], rec["result"] = r["avg"].view(f32), r["result"].view(f32)  # stored as raw bits
                rec["eigenvalues"] = r["eigenvalues"].view(f64)
            for a in rec.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            out[case] = rec
        _loaded = (out, json.loads(str(z["environment"])))
    return _loaded[0]


def environment():
    load()
    return _loaded[1]
