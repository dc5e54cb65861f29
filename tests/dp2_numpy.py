"""Integer / float64 numpy restatement of the reference's DPPratiMediodBGS and DPTextureBGS (package_bgs/dp: PratiMediodBGS.cpp,
TextureBGS.cpp and their DP*BGS.cpp wrappers) - the CPU yardstick of BGS_DP_PRATI_MEDIOD and BGS_DP_TEXTURE (not a test module).

Every step is the reference's own, in its order: PratiMediod's Subtract before Update, the stale old slot inside UpdateMediod, the
first strict minimum in slot order; Texture's LBP with HYSTERSIS, the 11x11 histograms, proximity < 181.5, the r-only update in
double and its gate fgMask(x, y) read at flat byte x * widthStep + y of the mask image (a byte past the image or in
row padding reads as 0).  tests/golden/dp2_ref_*.npz (outputs of the reference's own code) pin it; the GPU tests compare the engine's
masks and model planes with it.

Both classes can follow a subset of the pixels (`pixels`: flat indices) so that 1080p clips stay cheap: PratiMediod then also
follows their 8 neighbours, Texture the transposed pixels its update gate reads.
"""
import zlib

import numpy as np

REGION_R, TEXTURE_R, HYSTERSIS = 5, 2, 3
EDGE = REGION_R + TEXTURE_R               # 7: only 7 <= x < W-7, 7 <= y < H-7 are processed
ALPHA = float(np.float32(0.05))           # const double ALPHA = 0.05f
THRESHOLD = 0.5 * 11 * 11 * 3             # 181.5


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def linf(a, b):
    """L-inf distance of [..., 3] uint8 pixels, as int64."""
    return np.abs(a.astype(np.int64) - b.astype(np.int64)).max(-1)


class Prati:
    """DPPratiMediodBGS: threshold = LowThreshold (HighThreshold = 2x), sampling_rate, history_size.  process() -> the mask
    (uint8, 0 / 255) at the followed pixels (whole frame by default; other pixels 0)."""

    def __init__(self, threshold=30, sampling_rate=5, history_size=16, pixels=None):
        self.low, self.rate, self.H = int(threshold), int(sampling_rate), int(history_size)
        self.high = 2 * self.low
        self.pixels, self.fn = pixels, 0

    def _setup(self, rows, cols):
        self.rows, self.cols = rows, cols
        n = rows * cols
        want = np.arange(n) if self.pixels is None else np.asarray(self.pixels, np.int64)
        y, x = want // cols, want % cols
        nb = [want]
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                yy, xx = y + dy, x + dx
                ok = (yy >= 0) & (xx >= 0) & (yy < rows) & (xx < cols)
                nb.append((yy * cols + xx)[ok])
        self.track = want if self.pixels is None else np.unique(np.concatenate(nb))
        self.want = want
        self.look = np.full(n, -1, np.int64)
        self.look[self.track] = np.arange(len(self.track))
        K = len(self.track)
        self.samples = np.zeros((self.H, K, 3), np.uint8)
        self.dist = np.zeros((self.H, K), np.int64)
        self.median = np.zeros((K, 3), np.uint8)
        self.cnt, self.pos = 0, 0

    def process(self, frame):
        rows, cols = frame.shape[:2]
        if self.fn == 0:
            self._setup(rows, cols)
        cur = frame.reshape(-1, 3)[self.track]
        out = np.zeros(rows * cols, np.uint8)
        if self.fn >= self.H:  # Subtract: CalculateMasks with the medoid of the last update, then Combine
            d = linf(cur, self.median)
            low, high = d > self.low, d > self.high
            w = self.want
            y, x = w // cols, w % cols
            inner = (y > 0) & (x > 0) & (y < rows - 1) & (x < cols - 1)
            wi = self.look[w[inner]]
            m = high[wi].copy()
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dy or dx:
                        m |= low[wi] & high[self.look[w[inner] + dy * cols + dx]]
            out[w[inner]] = np.where(m, 255, 0)
        if self.fn % self.rate == 0:  # Update (the wrapper's update mask is all BACKGROUND)
            full = self.cnt == self.H
            n = self.cnt
            if full:
                old = self.samples[self.pos]
                self.dist[:n] -= linf(old[None], self.samples[:n])
            dd = linf(self.samples[:n], cur[None])
            self.dist[:n] += dd
            L = dd.sum(0)
            if n:
                k = np.argmin(self.dist[:n], 0)  # first strict minimum in slot order
                best = self.dist[:n][k, np.arange(len(k))]
                med = self.samples[:n][k, np.arange(len(k))]
                self.median = np.where((L < best)[:, None], cur, med)
            else:
                self.median = cur.copy()
            slot = self.pos if full else n
            self.dist[slot] = L
            self.samples[slot] = cur
            if full:
                self.pos = (self.pos + 1) % self.H
            else:
                self.cnt += 1
        self.fn += 1
        return out.reshape(rows, cols)

    def planes(self):
        """The engine's state planes of the followed pixels (whole frame: exactly bgs_get_state's)."""
        return {"samples": self.samples.copy(), "dist": self.dist.astype(np.uint16), "median": self.median.copy()}


def lbp(frame):
    """TextureBGS::LBP: [H, W, 3] 6-bit codes, 0 within TEXTURE_R of the border (the texture image is cvZero'd)."""
    f = frame.astype(np.int32)
    H, W = f.shape[:2]
    out = np.zeros(f.shape, np.uint8)
    if H <= 4 or W <= 4:
        return out
    c = f[2:H - 2, 2:W - 2] + HYSTERSIS
    code = np.zeros(c.shape, np.int32)
    for bit, (dy, dx) in enumerate(((-2, 0), (-1, -2), (-1, 2), (1, -2), (1, 2), (2, 0))):
        code |= (c >= f[2 + dy:H - 2 + dy, 2 + dx:W - 2 + dx]).astype(np.int32) << bit
    out[2:H - 2, 2:W - 2] = code
    return out


def histograms(codes, ys, xs):
    """11x11 window histograms at pixels (ys, xs): [K, 3, 64] uint8 in the reference's r, g, b order."""
    K = len(ys)
    if not K:
        return np.zeros((0, 3, 64), np.uint8)
    d = np.arange(-REGION_R, REGION_R + 1)
    win = codes[ys[:, None, None] + d[None, :, None], xs[:, None, None] + d[None, None, :]]  # [K, 11, 11, 3] (b, g, r)
    win = win[..., ::-1].reshape(K, -1, 3).astype(np.int64)  # r, g, b
    idx = np.arange(K)[:, None, None] * 192 + np.arange(3)[None, None, :] * 64 + win
    return np.bincount(idx.ravel(), minlength=K * 192).reshape(K, 3, 64).astype(np.uint8)


def histograms_at(frame, ys, xs):
    """The same histograms straight from the frame: LBP of each processed pixel's 15x15 patch (its window plus TEXTURE_R), so that a
    sample of a 1080p frame costs only its own pixels.  (ys, xs) must be processed pixels."""
    K = len(ys)
    if not K:
        return np.zeros((0, 3, 64), np.uint8)
    d = np.arange(-EDGE, EDGE + 1)
    f = frame[ys[:, None, None] + d[None, :, None], xs[:, None, None] + d[None, None, :]].astype(np.int32)  # [K, 15, 15, 3]
    c = f[:, 2:13, 2:13] + HYSTERSIS
    code = np.zeros(c.shape, np.int64)
    for bit, (dy, dx) in enumerate(((-2, 0), (-1, -2), (-1, 2), (1, -2), (1, 2), (2, 0))):
        code |= (c >= f[:, 2 + dy:13 + dy, 2 + dx:13 + dx]).astype(np.int64) << bit
    win = code[..., ::-1].reshape(K, -1, 3)  # r, g, b
    idx = np.arange(K)[:, None, None] * 192 + np.arange(3)[None, None, :] * 64 + win
    return np.bincount(idx.ravel(), minlength=K * 192).reshape(K, 3, 64).astype(np.uint8)


def r_update(cur, bg):
    """UpdateModel's (unsigned char)(ALPHA*cur + (1-ALPHA)*bg + 0.5), in double."""
    return (ALPHA * cur.astype(np.float64) + (1 - ALPHA) * bg.astype(np.float64) + 0.5).astype(np.uint8)


def gate_source(rows, cols, ys, xs):
    """Where fgMask(x, y) reads: flat byte x * widthStep + y of the 1-channel mask image.  Returns the flat pixel index it lands on,
    or -1 past the image or in row padding (read as 0: DESIGN.md §5.4)."""
    ws = (cols + 3) & ~3
    flat = xs.astype(np.int64) * ws + ys
    r, c = flat // ws, flat % ws
    return np.where((r < rows) & (c < cols), r * cols + c, -1)


class Texture:
    """DPTextureBGS.  process() -> the mask (uint8, 0 / 255) at the followed pixels (whole interior by default; other pixels 0)."""

    def __init__(self, pixels=None):
        self.pixels, self.fn = pixels, 0

    def _setup(self, rows, cols):
        self.rows, self.cols = rows, cols
        y, x = np.mgrid[0:rows, 0:cols]
        inter = ((y >= EDGE) & (x >= EDGE) & (y < rows - EDGE) & (x < cols - EDGE)).ravel()
        if self.pixels is None:
            track = np.nonzero(inter)[0]
        else:
            p = np.asarray(self.pixels, np.int64)
            p = p[inter[p]]
            g = gate_source(rows, cols, p // cols, p % cols)
            g = g[g >= 0]
            track = np.unique(np.concatenate([p, g[inter[g]]]))  # the transposed pixels the gates read
        self.track = track
        self.ys, self.xs = track // cols, track % cols
        self.look = np.full(rows * cols, -1, np.int64)
        self.look[track] = np.arange(len(track))
        self.gsrc = gate_source(rows, cols, self.ys, self.xs)
        self.model = None

    def process(self, frame):
        rows, cols = frame.shape[:2]
        if self.fn == 0:
            self._setup(rows, cols)
        cur = histograms_at(frame, self.ys, self.xs)
        if self.model is None:
            self.model = cur.copy()
        prox = np.minimum(self.model, cur).astype(np.int64).sum((1, 2))
        m = np.where(prox < THRESHOLD, 255, 0).astype(np.uint8)
        out = np.zeros(rows * cols, np.uint8)
        out[self.track] = m
        # UpdateModel: gated by this frame's mask at the transposed byte; only r
        g = np.zeros(len(self.track), np.uint8)
        ok = self.gsrc >= 0
        g[ok] = out[self.gsrc[ok]]
        # (a gate on a pixel this run does not follow lies outside the interior: its mask byte is 0, as `out` holds)
        upd = g == 0
        self.model[upd, 0] = r_update(cur[upd, 0], self.model[upd, 0])
        self.fn += 1
        return out.reshape(rows, cols)

    def hist_plane(self):
        """bgs_get_state "hist": [n, 3, 64], 0 outside the followed pixels."""
        out = np.zeros((self.rows * self.cols, 3, 64), np.uint8)
        out[self.track] = self.model
        return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Seeded clips of the fixtures (tests/golden/dp2_ref_*.npz store each one's CRC-32)

def scene_clip(T, H, W, seed, box=0.2, noise=3, speed=(1, 2)):
    """Static textured background with +-noise sensor noise and a moving flat box of about `box` of the area."""
    rng = np.random.default_rng(seed)
    base = rng.integers(30, 220, (H, W, 3), dtype=np.int16)
    bh, bw = max(int(H * np.sqrt(box)), 1), max(int(W * np.sqrt(box)), 1)
    out = np.empty((T, H, W, 3), np.uint8)
    for t in range(T):
        f = base + rng.integers(-noise, noise + 1, (H, W, 3), dtype=np.int16)
        y, x = (t * speed[0]) % max(H - bh, 1), (t * speed[1]) % max(W - bw, 1)
        f[y:y + bh, x:x + bw] = (230, 40, 90)
        out[t] = np.clip(f, 0, 255)
    return out


def tie_clip(T, H, W, seed):
    """Saturated, tie-heavy input: every byte 0, 128 or 255, many exact repeats, so equal distance sums are common."""
    rng = np.random.default_rng(seed)
    vals = np.array([0, 255, 128, 0, 255], np.uint8)
    base = vals[rng.integers(0, len(vals), (H, W, 3))]
    out = np.empty((T, H, W, 3), np.uint8)
    for t in range(T):
        f = base.copy()
        flip = rng.random((H, W)) < 0.3
        f[flip] = vals[rng.integers(0, len(vals), (int(flip.sum()), 3))]
        out[t] = f
    return out


def texture_clip(T, H, W, seed):
    """Textured background with noise and a moving box of a different texture (stripes), for DPTextureBGS."""
    rng = np.random.default_rng(seed)
    base = rng.integers(40, 200, (H, W, 3), dtype=np.int16)
    yy, xx = np.mgrid[0:H, 0:W]
    stripes = np.where(((xx + yy) // 2) % 2 == 0, 220, 20).astype(np.int16)
    bh, bw = max(H // 3, 1), max(W // 3, 1)
    out = np.empty((T, H, W, 3), np.uint8)
    for t in range(T):
        f = base + rng.integers(-4, 5, (H, W, 3), dtype=np.int16)
        y, x = (t * 2) % max(H - bh, 1), (t * 1) % max(W - bw, 1)
        f[y:y + bh, x:x + bw] = stripes[y:y + bh, x:x + bw, None]
        out[t] = np.clip(f, 0, 255)
    return out
