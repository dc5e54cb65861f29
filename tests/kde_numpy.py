"""Float64 numpy restatement of the reference's KDE class (package_bgs/ae: KDE.cpp, NPBGSubtractor.cpp, NPBGmodel.cpp,
KernelTable.cpp) - the CPU yardstick of BGS_KDE (not a test module).

Every arithmetic step is the reference's own, in the same order and precision: the kernel table through the C library's exp
(math.exp), the early-exit density loop as a sequential accumulation over the still-active pixels (sum < th*SL), p = sum / j
and p > Threshold.  tests/golden/kde_ref*.npz (masks of the reference's own code) pin it; the GPU tests compare the engine's
masks and model planes with it.
"""
import math

import numpy as np

HALF = 255            # KERNELHALFWIDTH
SMIN, SMAX, SBINS = 0.5, 36.5, 80
ABS_BINS = 20         # Estimation(): Abshistbins
RESET_MASK_TH = 500   # NPBGmodel bg_suppression_time


def kernel_table():
    """KernelLUTable(255, 0.5, 36.5, 80): [80][511] float64 (KernelTable.cpp:60-116, PI = 3.14159)."""
    PI = 3.14159
    tab = np.zeros((SBINS, 2 * HALF + 1))
    step = (SMAX - SMIN) / SBINS
    segma = SMIN
    for b in range(SBINS):
        c1 = 1 / (math.sqrt(2 * PI) * segma)
        c2 = -1 / (2 * segma * segma)
        s = 0.0
        row = [0.0] * (HALF + 1)
        for x in range(HALF + 1):
            y = x / 1.0
            v = c1 * math.exp(c2 * y * y)
            row[x] = v
            s += 2 * v
        s -= c1
        for x in range(HALF + 1):
            v = row[x] / s
            tab[b, HALF + x] = v
            tab[b, HALF - x] = v
        segma += step
    return tab


_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = kernel_table()
    return _TABLE


def gate_table(alpha):
    """(x1, x2) of the colour-ratio brightness gate for every sample brightness g (NPBGSubtractor.cpp:966-985)."""
    out = np.zeros((256, 2), np.int32)
    beta, betau = 3.0, 100.0
    for g in range(256):
        if g < beta / alpha:
            x1, x2 = int(g - beta), int(g + beta)
        elif g > betau / alpha:
            x1, x2 = int(g - betau), int(g + betau)
        else:
            x1, x2 = int(g * (1 - alpha) + 0.5), int(g * (1 + alpha) + 0.5)
        out[g] = x1, x2
    return out


def bgr2sngnrn(img):
    """BGR2SnGnRn (NPBGSubtractor.cpp:64-90) of [..., 3] uint8."""
    b, g, r = (img[..., k].astype(np.uint32) for k in range(3))
    s = 255.0 / (b + g + r + 30).astype(np.float64)
    r2 = ((g + 10) * s).astype(np.uint32)
    r3 = ((r + 10) * s).astype(np.uint32)
    out = np.empty(img.shape, np.uint8)
    out[..., 0] = ((b + g + r) // 3).astype(np.uint8)
    out[..., 1] = np.minimum(r2, 255).astype(np.uint8)
    out[..., 2] = np.minimum(r3, 255).astype(np.uint8)
    return out


def sd_bins(seq, estimate=True):
    """Estimation(): SD bin per (pixel, channel) from the 20-bin |slot i - slot i-1| histograms of the whole sequence
    (BuildAbsDiffHist, FindHistMedians, EstimateSDsFromAbsDiffHist).  seq: [SL][N][C] uint8."""
    SL = seq.shape[0]
    if not estimate:
        return np.full(seq.shape[1:], int(math.floor(((1.0 - SMIN) * SBINS) / (SMAX - SMIN))), np.uint8)
    d = np.abs(seq[1:].astype(np.int16) - seq[:-1].astype(np.int16))
    bins = np.minimum(d, ABS_BINS - 1).astype(np.uint8).reshape(SL - 1, -1).T  # [N*C][SL-1]
    mc = (SL - 1) // 2  # medianCount
    srt = np.sort(bins, axis=1)
    b = srt[:, mc - 1]  # the median bin: the first whose running count reaches medianCount
    x2 = (srt <= b[:, None]).sum(1).astype(np.float64)  # AccSum
    x1 = (srt < b[:, None]).sum(1).astype(np.float64)  # AccSum minus the median bin's count
    b, x1, x2 = (a.reshape(seq.shape[1:]) for a in (b, x1, x2))
    v = 1.04 * (b.astype(np.float64) - (x2 - mc) / (x2 - x1))
    v = np.where(v <= SMIN, SMIN, v)
    factor = (SBINS - 1) / (SMAX - SMIN)
    out = np.where(v >= SMAX, SBINS - 1, np.floor((v - SMIN) * factor + .5))
    return out.astype(np.uint8)


class Kde:
    """One reference KDE object (one stream): process(frame) -> mask uint8 [rows][cols], or None on a learning frame."""

    def __init__(self, frames_to_learn=10, sequence_length=50, time_window=100, sd_estimation=1, color_ratios=1, threshold=10e-8,
                 alpha=0.3, update_model=1):
        self.F, self.SL, self.TW = frames_to_learn, sequence_length, time_window
        self.sdf, self.cr, self.th, self.alpha, self.update = sd_estimation, color_ratios, threshold, alpha, update_model
        self.first = True
        self.trips = 0       # density-loop trips over every subtracted pixel so far
        self.lanes = 0

    def _init(self, shape):
        self.rows, self.cols = shape[:2]
        self.C = 1 if len(shape) == 2 else shape[2]
        N = self.rows * self.cols
        self.TBL = max(self.TW // self.SL, 2) & 0xFF  # NPBGmodel::TemporalBufferLength is an unsigned char
        self.seq = np.zeros((self.SL, N, self.C), np.uint8)
        self.qtop = np.zeros(N, np.uint8)
        self.tb = np.zeros((self.TBL, N, self.C), np.uint8)
        self.tmask = np.zeros((self.TBL, N), np.uint8)
        self.acc = np.zeros(N, np.uint32)
        self.sd = np.zeros((N, self.C), np.uint8)
        self.fn = self.top = self.tidx = self.tbc = self.tbtop = 0
        self.gate = gate_table(self.alpha)
        self.first = False

    def convert(self, frame):
        x = frame.reshape(-1, self.C)
        return bgr2sngnrn(x) if (self.cr and self.C == 3) else x.copy()

    def process(self, frame):
        if self.first:
            self._init(frame.shape)
        if self.fn < self.F:  # AddFrame
            x = self.convert(frame)
            self.seq[self.top] = x
            self.top = (self.top + 1) % self.SL
            self.qtop[:] = self.top
            self.tb[0] = x
            self.fn += 1
            return None
        if self.fn == self.F:  # Estimation
            self.tmask[:] = 0
            self.acc[:] = 0
            self.sd = sd_bins(self.seq, bool(self.sdf))
            self.tidx = 0
            self.fn += 1
        x = self.convert(frame)
        fg = self.subtract(x)
        if self.update:
            self._update(x, fg)
        return fg.reshape(self.rows, self.cols)

    def subtract(self, x):
        """The early-exit loop `while (j < SL && sum < th*SL) { sum += term; j++ }` over the pixels still in it."""
        K = table().ravel()
        N, SL = x.shape[0], self.SL
        th_sum = self.th * SL
        xi = x.astype(np.int64)
        kb = self.sd.astype(np.int64) * (2 * HALF + 1) + HALF - xi  # K[sd][g - x + HALF] = K.ravel()[kb + g]
        s = np.zeros(N)
        j = np.zeros(N, np.int64)
        live = np.arange(N) if th_sum > 0 else np.zeros(0, np.int64)
        for t in range(SL):
            if not len(live):
                break
            full = len(live) == N
            g = (self.seq[t] if full else self.seq[t, live]).astype(np.int64)
            kl = kb if full else kb[live]
            if self.C == 1:
                term = K.take(kl[:, 0] + g[:, 0])
            elif self.cr:
                xl = xi[:, 0] if full else xi[live, 0]
                ok = (self.gate[g[:, 0], 0] < xl) & (xl < self.gate[g[:, 0], 1])
                term = np.where(ok, K.take(kl[:, 1] + g[:, 1]) * K.take(kl[:, 2] + g[:, 2]), 0.0)
            else:
                term = (K.take(kl[:, 0] + g[:, 0]) * K.take(kl[:, 1] + g[:, 1])) * K.take(kl[:, 2] + g[:, 2])
            s[live] += term
            j[live] += 1
            live = live[s[live] < th_sum]
        self.trips += int(j.sum())
        self.lanes += N
        with np.errstate(invalid="ignore", divide="ignore"):
            p = s / j  # j = 0 only when th <= 0: 0 / 0 = NaN, not > th, so foreground (as in the reference)
        return np.where(p > self.th, 0, 255).astype(np.uint8)

    def _update(self, x, fg):
        """SequenceBGUpdate_Pairs (NPBGSubtractor.cpp:664-851); fg is zeroed in place where AccMask passes ResetMaskTh."""
        SL, TBL = self.SL, self.TBL
        rate = max(self.TW // SL, 2)
        top, nxt = self.tbtop, (self.tbtop + 1) % TBL
        if self.tidx % rate == 0 and self.tbc >= TBL:
            keep = (self.tmask[top] == 0) & (self.tmask[nxt] == 0)
            idx = np.nonzero(keep)[0]
            q = self.qtop[idx].astype(np.int64)
            self.seq[q, idx] = self.tb[top, idx]
            self.seq[(q + 1) % SL, idx] = self.tb[nxt, idx]
            self.qtop[idx] = ((q + 2) % SL).astype(np.uint8)
        self.tb[top] = x
        self.acc = np.where(fg != 0, self.acc + 1, 0).astype(np.uint32)
        fg[self.acc > RESET_MASK_TH] = 0
        self.tmask[top] = fg
        self.tbtop = (top + 1) % TBL
        self.tbc += 1
        self.tidx += 1

    def planes(self):
        """The model as bgs_get_state reads it back: samples [SL][N][C], sd_bins [N][C], qtop [N], acc [N]."""
        return {"samples": self.seq, "sd_bins": self.sd, "qtop": self.qtop, "acc": self.acc}


def long_clip(T=540, rows=16, cols=16, seed=7):
    """Seeded BGR clip of the AccMask case: a static noisy scene whose 6x6 block at (4, 5) turns a novel colour at frame 20 and
    keeps it (plus noise) to the end, so that it is foreground for > 500 consecutive frames, is then suppressed
    (ResetMaskTh) and relearnt by the update."""
    rng = np.random.default_rng(seed)
    base = rng.integers(40, 120, (rows, cols, 3))
    noise = rng.integers(-2, 3, (T, rows, cols, 3))
    clip = base[None] + noise
    clip[20:, 4:10, 5:11] = np.array([30, 60, 220]) + noise[20:, 4:10, 5:11]
    return np.clip(clip, 0, 255).astype(np.uint8)
