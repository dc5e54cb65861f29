"""float64 numpy restatement of the reference's five package_bgs/lb/ models (BGModelGauss, BGModelFuzzyGauss, BGModelMog,
BGModelSom, BGModelFuzzySom behind their LB*.cpp wrappers) - the CPU yardstick of BGS_LB_* (not a test module).

Vectorised over pixels, explicit loops over the K modes and the 3 x 3 neurons in the reference's order.  Every expression keeps the
reference's order of operations - distances sum the Red term first, (byte 2 + byte 1) + byte 0 - because in double the order decides
the last bit and with it `d2 < threshold` at ties.  numpy's elementwise + - * / sqrt on float64 are IEEE operations, one rounding
each, nothing fused.  tests/golden/lb_ref_*.npz (outputs of the reference's own code) pin it; the GPU tests compare the engine with it.

The wrapper's order is kept: the first frame runs Init() with the constructor's noise (50) BEFORE the first setBGModelParameter,
then every frame sets the parameters from the 0..255 integers and runs Update().

exp(): the two fuzzy models call it once per pixel and frame.  `exp=` selects the implementation: the default is libm's, called
value by value (numpy's own vectorised exp is a third implementation and deliberately not used); the tests also pass versions nudged
one ulp up / down to measure how far a last-bit difference of exp() can move the model (FUZZY_PLANE_TOL below).
"""
import math
import zlib

import numpy as np

SIMPLE_GAUSSIAN, FUZZY_GAUSSIAN, MOG, ADAPTIVE_SOM, FUZZY_ADAPTIVE_SOM = 25, 26, 27, 28, 29  # USTC_BGS types
NAMES = {25: "LBSimpleGaussian", 26: "LBFuzzyGaussian", 27: "LBMixtureOfGaussians", 28: "LBAdaptiveSOM", 29: "LBFuzzyAdaptiveSOM"}
FIELDS = ("sensitivity", "bg_threshold", "learning_rate", "noise_variance", "training_sensitivity", "training_learning_rate", "training_steps")
DEFAULTS = {  # LB*.cpp:19-20
    25: dict(sensitivity=66, noise_variance=162, learning_rate=18),
    26: dict(sensitivity=72, bg_threshold=162, learning_rate=49, noise_variance=195),
    27: dict(sensitivity=81, bg_threshold=83, learning_rate=59, noise_variance=206),
    28: dict(sensitivity=75, training_sensitivity=245, learning_rate=62, training_learning_rate=255, training_steps=55),
    29: dict(sensitivity=90, training_sensitivity=240, learning_rate=38, training_learning_rate=255, training_steps=81),
}
NOISE0 = 50.0                          # NOISEGAUSS / NOISEFUZZYGAUSS / INITIALVARMOG: what Init() sees
LEARNINGRATEMOG = float(np.float32(0.001))  # the weight of a new mode: the float constant widened, not m_alpha
FUZZYEXP, FUZZYTHRESH = -5.0, 0.8
DBL_MIN = np.finfo(np.float64).tiny
WMAX = 4.0                             # largest entry of the Pascal kernel (1 2 1) x (1 2 1)
PASCAL = np.array([[1.0, 2.0, 1.0], [2.0, 4.0, 2.0], [1.0, 2.0, 1.0]])

# Tolerance of the fuzzy classes' model planes on the GPU (absolute; "mu" / "som" live in 0..255, "var" in 0..255^2).
# Derivation: tests/test_lb_cpu.py runs the restatement on every fuzzy fixture with exp() nudged one ulp up and one
# ulp down on every call and takes D = the largest absolute deviation of a model plane from the REFERENCE fixture (it depends on
# the reference and this restatement only, not on the code under test), kept per plane because mu and var differ in scale:
#   LBFuzzyGaussian     mu  D = 4.3e-13 (1.7e-15 x 255)     var D = 4.0e-11 (6.2e-16 x 255^2)     (both from the case ties_fast)
#   LBFuzzyAdaptiveSOM  som D = 5.7e-14 (2.2e-16 x 255)
# glibc's and the device library's exp() are each within about an ulp of the true value, so they differ by at most two per call,
# and a same-direction nudge on every call is already the adverse pattern; a further factor 2 covers rounding that diverges once
# inputs differ: tolerance = 4 x D, rounded up to one digit.  The CPU test prints D and fails if a constant is below 4 D or above
# 40 D, so a stale constant is noticed.  In both nudged runs no mask bit and no background byte of any fixture moves, which is what
# entitles the GPU tests to compare the fuzzy classes' masks and background bytes exactly.
FUZZY_PLANE_TOL = {26: {"mu": 2e-12, "var": 2e-10}, 29: {"som": 3e-13}}

_libm_exp = np.frompyfunc(math.exp, 1, 1)


def libm_exp(x):
    return _libm_exp(x).astype(np.float64)


def exp_up(x):
    return np.nextafter(libm_exp(x), np.inf)


def exp_down(x):
    return np.nextafter(libm_exp(x), -np.inf)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def model_params(p):
    """setBGModelParameter of the five models: the 0..255 integers -> doubles, in the reference's order of operations."""
    dv = lambda v: float(v) / 255.0  # noqa: E731
    m = {}
    d = dv(p["sensitivity"])
    m["threshold"] = 100.0 * d * d
    m["eps2"] = 255.0 * 255.0 * d * d * d * d
    d = dv(p["training_sensitivity"])
    m["eps1"] = 255.0 * 255.0 * d * d * d * d
    m["noise"] = 100.0 * dv(p["noise_variance"])
    d = dv(p["learning_rate"])
    m["alpha"] = d * d * d
    m["alpha2"] = d * d * d / WMAX
    d = dv(p["training_learning_rate"])
    m["alpha1"] = d * d * d / WMAX
    m["bg_threshold"] = dv(p["bg_threshold"])
    m["tsteps"] = int(255.0 * dv(p["training_steps"]))
    return m


def _step(m, a, d):
    """`if (d*d > DBL_MIN) m += a*d`"""
    return np.where(d * d > DBL_MIN, m + a * d, m)


def _trunc(x):
    return x.astype(np.int64).astype(np.uint8)  # (unsigned char) of a double in 0..255


class LB:
    """One LB* object: cls = USTC_BGS type 25..29, keyword parameters = the wrapper's integers (defaults: the constructor's).
    process(frame) -> (mask uint8 0 / 255 [rows][cols], background uint8 [rows][cols][3]).  `pixels`: follow only these flat indices
    (the other pixels of the outputs are 0) so that 1080p clips stay cheap.  set(**kw) changes parameters between frames, like an
    edited XML."""

    def __init__(self, cls, exp=None, pixels=None, **kw):
        self.cls = int(cls)
        self.p = {k: 0 for k in FIELDS}
        self.p.update(DEFAULTS[self.cls])
        self.set(**kw)
        self.exp = exp or libm_exp
        self.pixels, self.fn, self.K = pixels, 0, 0
        self.swaps = 0       # MoG: sort swaps so far (fixture sanity)
        self.first_not_best = 0  # MoG: matches whose first hit was not the nearest mode
        self.replaced = 0    # MoG: new modes that replaced the last slot of a full pixel
        self.bmu_seen = set()  # SOMs: "corner" / "edge" / "centre" BMUs of matched pixels so far

    def set(self, **kw):
        for k, v in kw.items():
            assert k in FIELDS, k
            self.p[k] = int(v)

    # -- Init() ------------------------------------------------------------------------------------------------------------
    def _init(self, src):
        n = len(src)
        if self.cls in (25, 26):
            self.mu, self.var = src.copy(), np.full((n, 3), NOISE0)
        elif self.cls == 27:
            self.w, self.mu, self.var = np.zeros((n, 3)), np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
            self.mu[:, 0], self.var[:, 0], self.w[:, 0] = src, NOISE0, 1.0
            self.k = np.ones(n, np.int32)
        else:
            self.som = np.repeat(src[:, None, :], 9, 1).reshape(n, 3, 3, 3).copy()
            self.bg = np.zeros((n, 3), np.uint8)
            self.K = 0

    def process(self, frame):
        rows, cols = frame.shape[:2]
        flat = frame.reshape(-1, 3)
        idx = np.arange(rows * cols) if self.pixels is None else np.asarray(self.pixels, np.int64)
        src = flat[idx].astype(np.float64)
        if self.fn == 0:
            self._init(src)
        m = model_params(self.p)
        with np.errstate(all="ignore"):
            fg, bg = {25: self._gauss, 26: self._gauss, 27: self._mog, 28: self._som, 29: self._som}[self.cls](src, m)
        self.fn += 1
        ofg, obg = np.zeros(rows * cols, np.uint8), np.zeros((rows * cols, 3), np.uint8)
        ofg[idx], obg[idx] = fg, bg
        return ofg.reshape(rows, cols), obg.reshape(rows, cols, 3)

    # -- BGModelGauss::Update / BGModelFuzzyGauss::Update ------------------------------------------------------------------
    def _gauss(self, src, m):
        fuzzy = self.cls == 26
        mu, var = self.mu, self.var
        d = src - mu
        d2 = d[:, 2] * d[:, 2] / var[:, 2] + d[:, 1] * d[:, 1] / var[:, 1] + d[:, 0] * d[:, 0] / var[:, 0]
        if fuzzy:
            fz = np.where(d2 < m["threshold"], d2 / m["threshold"], 1.0)
            alpha = (m["alpha"] * self.exp(FUZZYEXP * fz))[:, None]
        else:
            alpha = m["alpha"]
        mu[:] = _step(mu, alpha, d)
        e = src - mu
        var[:] = _step(var, alpha, e * e - var)
        var[:] = np.maximum(var, m["noise"]) if fuzzy else np.minimum(var, m["noise"])  # BGModelGauss.cpp:182-184: a ceiling
        fg = (fz >= m["bg_threshold"]) if fuzzy else ~(d2 < m["threshold"])
        return np.where(fg, 255, 0).astype(np.uint8), _trunc(mu)

    # -- BGModelMog::Update --------------------------------------------------------------------------------------------------
    def _mog(self, src, m):
        n = len(src)
        w, mu, var, K = self.w, self.mu, self.var, self.k
        alpha, noise = m["alpha"], m["noise"]
        hit = np.full(n, -1)
        best, bestd = np.full(n, -1), np.full(n, np.inf)
        for k in range(3):  # the first mode within the threshold
            d = src - mu[:, k]
            safe = np.where(var[:, k] == 0, 1.0, var[:, k])
            d2 = d[:, 2] * d[:, 2] / safe[:, 2] + d[:, 1] * d[:, 1] / safe[:, 1] + d[:, 0] * d[:, 0] / safe[:, 0]
            hit = np.where((hit < 0) & (k < K) & (d2 < m["threshold"]), k, hit)
            nearer = (k < K) & (d2 < bestd)
            best, bestd = np.where(nearer, k, best), np.where(nearer, d2, bestd)
        matched = hit >= 0
        self.first_not_best += int((matched & (hit != best)).sum())
        for k in range(3):
            live = matched & (k < K)
            isk = live & (hit == k)
            w[:, k] = np.where(isk, w[:, k] + alpha * (1.0 - w[:, k]), np.where(live, (1.0 - alpha) * w[:, k], w[:, k]))
            nm = _step(mu[:, k], alpha, src - mu[:, k])
            e = src - nm
            nv = np.maximum(_step(var[:, k], alpha, e * e - var[:, k]), noise)
            mu[:, k] = np.where(isk[:, None], nm, mu[:, k])
            var[:, k] = np.where(isk[:, None], nv, var[:, k])
        new = ~matched  # a new mode; with all three in use the last one is replaced
        self.replaced += int((new & (K == 3)).sum())
        K[:] = np.where(new & (K < 3), K + 1, K)
        hit = np.where(new, K - 1, hit)
        for k in range(3):
            isk = new & (hit == k)
            w[:, k] = np.where(isk, np.where(K == 1, 1.0, LEARNINGRATEMOG), w[:, k])
            mu[:, k] = np.where(isk[:, None], src, mu[:, k])
            var[:, k] = np.where(isk[:, None], noise, var[:, k])
        wsum = np.zeros(n)
        for k in range(3):
            wsum = np.where(k < K, wsum + w[:, k], wsum)
        wf = 1.0 / wsum
        key = np.zeros((n, 3))
        for k in range(3):
            live = k < K
            w[:, k] = np.where(live, w[:, k] * wf, w[:, k])
            vs = var[:, k, 2] + var[:, k, 1] + var[:, k, 0]
            key[:, k] = np.where(live, w[:, k] / np.sqrt(np.where(live, vs, 1.0)), key[:, k])
        khit = key[np.arange(n), hit]
        sw = np.full(n, -1)
        for k in range(2):  # one swap towards the front
            sw = np.where((sw < 0) & (k < hit) & (khit > key[:, k]), k, sw)
        rows_ = np.nonzero(sw >= 0)[0]
        self.swaps += len(rows_)
        a, b = sw[rows_], hit[rows_]
        for arr in (w, key):
            arr[rows_, a], arr[rows_, b] = arr[rows_, b].copy(), arr[rows_, a].copy()
        for arr in (mu, var):
            arr[rows_, a], arr[rows_, b] = arr[rows_, b].copy(), arr[rows_, a].copy()
        acc, kbg, found = np.zeros(n), np.full(n, 2), np.zeros(n, bool)
        for k in range(3):
            live = (k < K) & ~found
            acc = np.where(live, acc + w[:, k], acc)
            now = live & (acc > m["bg_threshold"])
            kbg, found = np.where(now, k, kbg), found | now
        assert found.all()  # m_T < 1: the reference's kBG is always assigned
        return np.where(hit > kbg, 255, 0).astype(np.uint8), _trunc(mu[:, 0])  # kHit: the slot index from before the swap

    # -- BGModelSom::Update / BGModelFuzzySom::Update ------------------------------------------------------------------------
    def _som(self, src, m):
        fuzzy = self.cls == 29
        n = len(src)
        if self.K <= m["tsteps"]:  # calibration phase (frame 1 counts)
            eps = m["eps1"]
            alpha = m["alpha1"] - self.K * (m["alpha1"] - m["alpha2"]) / m["tsteps"]
            self.K += 1
        else:
            eps, alpha = m["eps2"], m["alpha2"]
        som = self.som
        d2min, hit = np.full(n, np.finfo(np.float64).max), np.zeros(n, np.int64)
        for l in range(3):
            for k in range(3):
                d = src - som[:, l, k]
                d2 = d[:, 2] * d[:, 2] + d[:, 1] * d[:, 1] + d[:, 0] * d[:, 0]
                better = d2 < d2min
                d2min, hit = np.where(better, d2, d2min), np.where(better, 3 * l + k, hit)
        hl, hk = hit // 3, hit % 3
        if fuzzy:
            fz = np.where(d2min < eps, d2min / eps if eps else 1.0, 1.0)
            rate = alpha * self.exp(FUZZYEXP * fz)
            update, isbg = np.ones(n, bool), ~(fz >= FUZZYTHRESH)
        else:
            rate = np.full(n, alpha)
            update = isbg = d2min <= eps
        for l in range(3):
            for k in range(3):
                dl, dk = l - hl, k - hk
                inw = update & (np.abs(dl) <= 1) & (np.abs(dk) <= 1)
                wgt = PASCAL[np.clip(dl + 1, 0, 2), np.clip(dk + 1, 0, 2)]
                a = (rate * wgt)[:, None]
                som[:, l, k] = np.where(inw[:, None], _step(som[:, l, k], a, src - som[:, l, k]), som[:, l, k])
        kinds = np.where((hl == 1) & (hk == 1), 2, np.where((hl == 1) | (hk == 1), 1, 0))[update]
        self.bmu_seen |= {("corner", "edge", "centre")[v] for v in np.unique(kinds)}
        hitc = som[np.arange(n), hl, hk]
        self.bg = np.where(isbg[:, None], _trunc(hitc), self.bg)
        return np.where(isbg, 0, 255).astype(np.uint8), self.bg.copy()

    def planes(self):
        """The engine's state planes of the followed pixels (whole frame: exactly bgs_get_state's)."""
        if self.cls in (25, 26):
            return {"mu": self.mu.copy(), "var": self.var.copy()}
        if self.cls == 27:
            live = np.arange(3)[None, :] < self.k[:, None]
            vs = self.var[:, :, 2] + self.var[:, :, 1] + self.var[:, :, 0]
            with np.errstate(all="ignore"):
                key = np.where(live, self.w / np.sqrt(np.where(live, vs, 1.0)), 0.0)
            return {"w": self.w.copy(), "mu": self.mu.copy(), "var": self.var.copy(), "sortkey": key, "k": self.k.copy()}
        return {"som": self.som.copy(), "bg": self.bg.copy(), "count": np.array([self.K], np.int64)}


# ---- seeded clips (fixtures name them "kind:T:H:W:seed") --------------------------------------------------------------------------

def noisy_clip(T, H, W, seed, box=0.1):
    """A textured static scene with sensor noise and a box that moves across it."""
    rng = np.random.default_rng(seed)
    base = rng.integers(40, 200, (H, W, 3)).astype(np.int16)
    out = np.empty((T, H, W, 3), np.uint8)
    bh, bw = max(2, int(H * box ** 0.5)), max(2, int(W * box ** 0.5))
    for t in range(T):
        f = base + rng.integers(-6, 7, (H, W, 3))
        y, x = (t * 2) % max(1, H - bh), (t * 3) % max(1, W - bw)
        f[y:y + bh, x:x + bw] = rng.integers(0, 256, 3)
        out[t] = np.clip(f, 0, 255)
    return out


def modes_clip(T, H, W, seed):
    """Every pixel dwells on one of four colours of its own for a random stretch, with small noise: MoG reaches K = 3, replaces its
    last mode and re-sorts; a SOM pixel stays foreground for a while (the stale background byte shows) and matches units in the
    corner, on an edge and in the centre."""
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, (4, H, W, 3)).astype(np.int16)
    pal[1] = np.clip(pal[0] + rng.integers(-25, 26, (H, W, 3)), 0, 255)  # a near neighbour: first hit and best hit differ
    out = np.empty((T, H, W, 3), np.uint8)
    cur = np.zeros((H, W), np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    for t in range(T):
        change = rng.random((H, W)) < 0.12
        cur = np.where(change, rng.integers(0, 4, (H, W)), cur)
        f = pal[cur, yy, xx] + rng.integers(-3, 4, (H, W, 3))
        out[t] = np.clip(f, 0, 255)
    return out


def tie_clip(T, H, W, seed):
    """Values from {0, 128, 255} only, long constant stretches: exact ties, d*d guards at 0, variances at their clamp."""
    rng = np.random.default_rng(seed)
    lv = np.array([0, 128, 255], np.uint8)
    out = np.empty((T, H, W, 3), np.uint8)
    cur = lv[rng.integers(0, 3, (H, W, 3))]
    for t in range(T):
        change = rng.random((H, W, 1)) < 0.15
        cur = np.where(change, lv[rng.integers(0, 3, (H, W, 3))], cur)
        out[t] = cur
    return out
