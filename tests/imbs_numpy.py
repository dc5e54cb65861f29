"""numpy restatement of package_bgs/db IndependentMultimodalBGS (Bloisi and Iocchi's IMBS, USTC_BGS type 33's class), written from
imbs.cpp:98-724 and IndependentMultimodalBGS.cpp:13-36, plus the seeded clips, the cases and the reader of
tests/golden/imbs_ref.npz (not a test module).

Everything is integer except convertImageRGBtoHSV, which is float32 here where the reference is float.  areaThresholding is OpenCV
(findContours / moments / drawContours), which is not in the tree: its contract is the definition of DESIGN.md §5.10, restated twice,
as a Suzuki border follower with a polygon area and fill (`area_filter_follower`, the contract) and as the search-free quad form the
device uses (`area_filter_quads`); tests/test_imbs_cpu.py holds the two together.  putText is a no-op: until bgModel[0].isValid[0]
the mask and the background are zero images."""
import json
import os
import zlib

import numpy as np

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLASS_NAME = "IndependentMultimodalBGS"
DEFAULTS = dict(fps=10.0, fgThreshold=15, associationThreshold=5, samplingPeriod=500, minBinHeight=2, numSamples=30, alpha=0.65, beta=1.15,
                tau_s=60, tau_h=40, minArea=30.0, persistencePeriod=10000, morphologicalFiltering=0)  # imbs.hpp:43-56, fps of the wrapper
PLANE_PIXELS = 1024  # the state planes are stored for the cases of at most this many pixels
CONTROL = ("timestamp", "prev_timestamp", "prev_bg_frame_time", "bg_frame_counter", "numSamples", "samplingPeriod", "bg_reset", "sudden_change", "maxBgBins", "valid0")


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xffffffff


# ---------------------------------------------------------------------------------------------------------------- the area filter
D8 = [(0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1)]  # clockwise from east, y down


def _follow(f, i, j, i2, j2, nbd):
    """Suzuki and Abe, step 3: the border that starts at (i, j) with (i2, j2) the zero it was found from."""
    s = D8.index((i2 - i, j2 - j))
    found = None
    for k in range(8):
        d = (s + k) % 8
        y, x = i + D8[d][0], j + D8[d][1]
        if f[y, x] != 0:
            found = (y, x)
            break
    if found is None:
        f[i, j] = -nbd
        return [(i, j)]
    i1, j1 = found
    p2, p3, pts = (i1, j1), (i, j), []
    while True:
        s = D8.index((p2[0] - p3[0], p2[1] - p3[1]))
        east_zero, p4 = False, None
        for k in range(1, 9):
            d = (s - k) % 8
            y, x = p3[0] + D8[d][0], p3[1] + D8[d][1]
            if f[y, x] != 0:
                p4 = (y, x)
                break
            if d == 0:
                east_zero = True
        pts.append(p3)
        if east_zero:
            f[p3] = -nbd
        elif f[p3] == 1:
            f[p3] = nbd
        if p4 == (i, j) and p3 == (i1, j1):
            break
        p2, p3 = p3, p4
    return pts


def contours(mask):
    """RETR_LIST borders of a binary image whose one-pixel frame has been cleared: [(kind, points)]."""
    f = (np.asarray(mask) != 0).astype(np.int64)
    H, W = f.shape
    f[0, :] = f[-1, :] = 0
    f[:, 0] = f[:, -1] = 0
    out, nbd = [], 1
    for i in range(1, H - 1):
        for j in range(1, W - 1):
            if f[i, j] == 0:
                continue
            if f[i, j] == 1 and f[i, j - 1] == 0:
                nbd += 1
                out.append(("outer", _follow(f, i, j, i, j - 1, nbd)))
            elif f[i, j] >= 1 and f[i, j + 1] == 0:
                nbd += 1
                out.append(("hole", _follow(f, i, j, i, j + 1, nbd)))
    return out


def polygon_area2(pts):
    """Twice the polygon area through the points (moments().m00 is exact halves)."""
    a = 0
    for k in range(len(pts)):
        y0, x0 = pts[k]
        y1, x1 = pts[(k + 1) % len(pts)]
        a += x0 * y1 - x1 * y0
    return abs(a)


def polygon_cover(pts, shape):
    """The contour's own points and every lattice point inside the polygon through them (even-odd crossing of a ray to +x)."""
    cov = np.zeros(shape, bool)
    P = np.array(pts, np.int64)
    cov[P[:, 0], P[:, 1]] = True
    if len(pts) < 3:
        return cov
    y0, y1, x0, x1 = P[:, 0].min(), P[:, 0].max(), P[:, 1].min(), P[:, 1].max()
    gy, gx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    gy, gx = gy.reshape(-1, 1), gx.reshape(-1, 1)
    ay, ax = P[:, 0][None, :], P[:, 1][None, :]
    Pn = np.roll(P, -1, axis=0)
    by, bx = Pn[:, 0][None, :], Pn[:, 1][None, :]
    straddle = (ay <= gy) != (by <= gy)
    # x of the edge at height gy is ax + (gy - ay) (bx - ax) / (by - ay); the point is left of it  <=>  cross product sign, integers
    dy = by - ay
    lhs = (gx - ax) * dy
    rhs = (gy - ay) * (bx - ax)
    left = np.where(dy > 0, lhs < rhs, lhs > rhs)
    inside = (np.count_nonzero(straddle & left, axis=1) % 2 == 1).reshape(y1 - y0 + 1, x1 - x0 + 1)
    cov[y0:y1 + 1, x0:x1 + 1] |= inside
    return cov


def kept(area2, min_area, n_pixels):
    area = area2 / 2.0
    return not (area < min_area or area >= 0.6 * n_pixels)


def area_filter_follower(plane, min_area, stats=None):
    """areaThresholding by its definition: which pixels of `plane` (bool) survive."""
    H, W = plane.shape
    tmp = np.zeros((H, W), bool)
    if H >= 3 and W >= 3:
        for kind, pts in contours(plane):
            if stats is not None:
                stats.setdefault("areas2", []).append(polygon_area2(pts))  # doubled areas, in the order the borders are met
            if kept(polygon_area2(pts), min_area, H * W):
                tmp |= polygon_cover(pts, (H, W))
                if stats is not None:
                    stats["kept_" + kind] = stats.get("kept_" + kind, 0) + 1
            elif stats is not None:
                stats["dropped_" + kind] = stats.get("dropped_" + kind, 0) + 1
    return plane & tmp


def area_filter_follower_many(plane, min_areas):
    """[area_filter_follower(plane, a) for a in min_areas] with the borders traced and filled once, and the doubled areas."""
    H, W = plane.shape
    traced = [(polygon_area2(pts), pts) for _, pts in contours(plane)] if H >= 3 and W >= 3 else []
    covers, out = {}, []
    for a in min_areas:
        tmp = np.zeros((H, W), bool)
        for i, (area2, pts) in enumerate(traced):
            if kept(area2, a, H * W):
                if i not in covers:
                    covers[i] = polygon_cover(pts, (H, W))
                tmp |= covers[i]
        out.append(plane & tmp)
    return out, [area2 for area2, _ in traced]


def label(mask, conn8):
    """Components of the true pixels, each named by the raster index of its first pixel; -1 elsewhere."""
    H, W = mask.shape
    L = np.full((H, W), -1, np.int64)
    nb = D8 if conn8 else [(0, 1), (1, 0), (0, -1), (-1, 0)]
    for i in range(H):
        for j in range(W):
            if mask[i, j] and L[i, j] < 0:
                root = i * W + j
                L[i, j] = root
                stack = [(i, j)]
                while stack:
                    y, x = stack.pop()
                    for dy, dx in nb:
                        v, u = y + dy, x + dx
                        if 0 <= v < H and 0 <= u < W and mask[v, u] and L[v, u] < 0:
                            L[v, u] = root
                            stack.append((v, u))
    return L


def area_filter_quads(plane, min_area, stats=None):
    """The same filter without border following, as the device computes it (kernel_imbs.h)."""
    H, W = plane.shape
    n = H * W
    ones = plane.copy()
    ones[0, :] = ones[-1, :] = False
    ones[:, 0] = ones[:, -1] = False
    L1, L0 = label(ones, True).reshape(-1), label(~ones, False).reshape(-1)
    o = ones.reshape(-1)
    Q = np.zeros(n, np.int64)
    for y in range(H - 1):
        for x in range(W - 1):
            q = [y * W + x, y * W + x + 1, (y + 1) * W + x, (y + 1) * W + x + 1]
            on = [g for g in q if o[g]]
            ze = [g for g in q if not o[g]]
            if len(on) == 4:
                Q[L1[q[0]]] += 2
            elif len(on) == 3:
                Q[L1[on[0]]] += 1
                Q[L0[ze[0]]] += 1
            elif len(on) == 2 and o[q[0]] == o[q[3]]:
                Q[L0[ze[0]]] += 1
                Q[L0[ze[1]]] += 1
            else:
                Q[L0[ze[0]]] += 2
    A = np.zeros(n, np.int64)
    roots1 = [g for g in range(n) if o[g] and L1[g] == g]
    roots0 = [g for g in range(n) if not o[g] and L0[g] == g and g != 0]
    for g in roots1 + roots0:
        own = Q[g]
        if o[g]:
            c = g
        else:
            A[g] += own
            c = L1[g - W]
        while True:
            A[c] += own
            z = L0[c - 1]
            if z == 0:
                break
            A[z] += own
            c = L1[z - W]
    chain = {}
    for g in roots1:
        c, k = g, False
        while True:
            if kept(A[c], min_area, n):
                k = True
                break
            z = L0[c - 1]
            if z == 0:
                break
            if kept(A[z], min_area, n):
                k = True
                break
            c = L1[z - W]
        chain[g] = k
    out = np.zeros(n, bool)
    for g in range(n):
        if not o[g]:
            continue
        c = L1[g]
        s = chain[c]
        if s and stats is not None:
            stats["chain"] = stats.get("chain", 0) + 1
        if not s:
            parent = L0[c - 1]
            for nbp in (g - 1, g + 1, g - W, g + W):
                if not o[nbp] and L0[nbp] != parent and kept(A[L0[nbp]], min_area, n):
                    s = True
            if stats is not None:
                stats["own_hole" if s else "dropped"] = stats.get("own_hole" if s else "dropped", 0) + 1
        out[g] = s
    return out.reshape(H, W)


def morph3(img, dilate):
    """3x3 box erode / dilate of a bool image; cells outside the image never take part (morphologyDefaultBorderValue)."""
    H, W = img.shape
    pad = np.full((H + 2, W + 2), not dilate, bool)
    pad[1:-1, 1:-1] = img
    acc = pad[1:-1, 1:-1].copy()
    for dy in range(3):
        for dx in range(3):
            v = pad[dy:dy + H, dx:dx + W]
            acc = (acc | v) if dilate else (acc & v)
    return acc


# ------------------------------------------------------------------------------------------------------------------------ the model
def hsv_bytes(bgr):
    """convertImageRGBtoHSV (imbs.cpp:539-665) on [..., 3] uint8 B, G, R -> H, S, V bytes, float32 step for step."""
    b = bgr[..., 0].astype(np.int64)
    g = bgr[..., 1].astype(np.int64)
    r = bgr[..., 2].astype(np.int64)
    k = f32(1.0) / f32(255.0)
    fR, fG, fB = r.astype(f32) * k, g.astype(f32) * k, b.astype(f32) * k
    iMax = np.maximum(np.maximum(b, g), r)
    iMin = np.minimum(np.minimum(b, g), r)
    fMax, fMin = iMax.astype(f32) * k, iMin.astype(f32) * k
    # fMin / fMax / iMax of the if-tree are the plain extremes; the hue branch compares iMax == bR first, then bG
    with np.errstate(all="ignore"):
        fDelta = fMax - fMin
        fS = fDelta / fMax
        unit = f32(1.0) / (f32(6.0) * fDelta)
        hR = (fG - fB) * unit
        hG = f32(2.0) / f32(6.0) + (fB - fR) * unit
        hB = f32(4.0) / f32(6.0) + (fR - fG) * unit
        fH = np.where(iMax == r, hR, np.where(iMax == g, hG, hB)).astype(f32)
        fH = np.where(fH < 0, fH + f32(1.0), fH).astype(f32)
        fH = np.where(fH >= 1, fH - f32(1.0), fH).astype(f32)
        black = iMax == 0
        fH = np.where(black, f32(0), fH).astype(f32)
        fS = np.where(black, f32(0), fS).astype(f32)

        def tob(v):
            t = f32(0.5) + v * f32(255.0)
            t = np.where(np.isnan(t), f32(-1), t)  # (int)NaN is INT_MIN there, clipped to 0
            return np.clip(np.trunc(t), 0, 255).astype(np.uint8)

        out = np.stack([tob(fH), tob(fS), tob(fMax)], axis=-1)
    return out


class Model:
    def __init__(self, params, rows, cols, area_filter=area_filter_follower):
        p = dict(DEFAULTS, **{k: v for k, v in params.items() if k in DEFAULTS})
        self.p, self.rows, self.cols, self.n = p, rows, cols, rows * cols
        self.area_filter, self.stats = area_filter, {}
        n = self.n
        self.cap = int(p["numSamples"])
        self.ns, self.sp = int(p["numSamples"]), int(p["samplingPeriod"])
        self.minbin = int(p["minBinHeight"])
        self.M = self.ns // self.minbin
        self.alpha, self.beta = f32(p["alpha"]), f32(p["beta"])
        self.ts = self.prev_ts = 0.0
        self.pbft = self.bfc = 0
        self.bg_reset = self.sudden = False
        self.persist = np.zeros(n, np.uint32)
        self.bv, self.bh, self.bf = np.zeros((n, self.cap, 3), np.uint8), np.zeros((n, self.cap), np.uint8), np.zeros((n, self.cap), np.uint8)
        self.mv, self.mvalid = np.zeros((n, self.M, 3), np.uint8), np.zeros((n, self.M), np.uint8)
        self.mf, self.mc = np.zeros((n, self.M), np.uint8), np.zeros((n, self.M), np.uint8)
        self.sample = np.zeros((n, 3), np.uint8)
        self.bgimg = np.zeros((n, 3), np.uint8)

    # getFg + hsvSuppression
    def detect(self, px):
        n, M, thr = self.n, self.M, int(self.p["fgThreshold"])
        dt = self.ts - self.prev_ts
        active = np.ones(n, bool)
        isfg = np.ones(n, bool)
        cond = np.zeros(n, bool)
        pi = px.astype(np.int64)
        for s in range(M):
            valid = self.mvalid[:, s] != 0
            if s == 0:
                isfg[active & ~valid] = False
            active &= valid
            d = np.abs(self.mv[:, s].astype(np.int64) - pi).max(1)
            close = active & (d < thr)
            c1 = close & (self.mf[:, s] != 0)
            cond |= c1
            active &= ~c1
            c2 = close & ~c1
            isfg[c2] = False
            self.persist[c2] = 0
        lab = np.zeros(n, np.uint8)
        p180 = isfg & cond
        lab[p180] = 180
        self.persist[p180] = np.trunc(self.persist[p180].astype(np.float64) + dt).astype(np.uint32)
        over = p180 & (self.persist > int(self.p["persistencePeriod"]))
        lead = np.cumprod(self.mvalid != 0, axis=1).astype(bool)
        self.mf[over[:, None] & lead] = 0
        p255 = isfg & ~cond
        lab[p255] = 255
        self.persist[p255] = 0
        # hsvSuppression
        hi = hsv_bytes(px).astype(np.int64)
        active = lab != 0
        for s in range(M):
            active &= self.mvalid[:, s] != 0
            cand = active & (self.mf[:, s] == 0)
            hb = hsv_bytes(self.mv[:, s]).astype(np.int64)
            with np.errstate(all="ignore"):
                ratio = hi[:, 2].astype(f32) / hb[:, 2].astype(f32)
            sd = np.abs(hi[:, 1] - hb[:, 1])
            ad = np.abs(hi[:, 0] - hb[:, 0])
            hd = np.minimum(ad, 255 - ad)
            with np.errstate(invalid="ignore"):
                sh = cand & (hd <= int(self.p["tau_h"])) & (sd <= int(self.p["tau_s"])) & (ratio >= self.alpha) & (ratio < self.beta)
            lab[sh] = 80
            active &= ~sh
        return lab

    def filter_fg(self, lab):
        plane = (lab == 255).reshape(self.rows, self.cols)
        if int(plane.sum()) > self.n * 0.5:
            self.sudden = True
        if self.p["morphologicalFiltering"]:
            plane = morph3(morph3(plane, False), True)
            plane = morph3(morph3(plane, True), False)
        plane = self.area_filter(plane, float(self.p["minArea"]), self.stats).reshape(-1)
        out = np.where(plane, 255, 0).astype(np.uint8)
        out[lab == 180] = 180
        out[lab == 80] = 80
        return out

    def create_bg(self, k, fg):
        n, ns, cap, M = self.n, self.ns, self.cap, self.M
        px = self.sample
        pi = px.astype(np.int64)
        is255 = fg == 255
        if k == 0:
            self.bv[:, 0] = px
            self.bh[:, 0] = 1
            self.bh[:, 1:min(ns, cap)] = 0
            self.bf[:, 0] = is255
        else:
            pending = np.ones(n, bool)
            assoc = int(self.p["associationThreshold"])
            for s in range(min(k, cap)):
                bvs = self.bv[:, s].astype(np.int64)
                h = self.bh[:, s].astype(np.int64)
                match = pending & (np.abs(pi - bvs).max(1) <= assoc)
                new = pending & ~match & (h == 0)
                den = h + 1
                upd = ((bvs * h[:, None] + pi) // den[:, None]).astype(np.uint8)
                self.bv[match, s] = upd[match]
                self.bh[match, s] = np.minimum(h[match] + 1, 63)
                self.bf[match & is255, s] = 1
                self.bv[new, s] = px[new]
                self.bh[new, s] = 1
                self.bf[new, s] = is255[new]
                pending &= ~(match | new)
            if k == ns - 1:
                self.build(fg)
        if k == ns - 1:
            self.persist[:] = 0
            self.bg_reset, shrunk = False, self.bg_reset
            if self.sudden:
                if shrunk:  # see kernel_imbs.h: the engine restores only what changeBg divided
                    self.ns = int(self.ns * 3.)
                    self.sp = int(self.sp * 2.)
                self.sudden = False
            self.bgimg = self.mv[:, 0].copy()

    def build(self, fg):
        n, M, thr = self.n, self.M, int(self.p["fgThreshold"])
        ar = np.arange(n)
        index = np.zeros(n, np.int64)
        maxh = np.full(n, -1, np.int64)
        stopped = np.zeros(n, bool)
        is180 = fg == 180
        for s in range(min(self.ns, self.cap)):
            h = self.bh[:, s].astype(np.int64)
            z = ~stopped & (h == 0)
            zi = z & (index < M)
            self.mvalid[ar[zi], index[zi]] = 0
            stopped |= z
            stopped |= ~stopped & (index == M)
            ok = ~stopped & (h >= self.minbin)
            act = ok & is180
            if act.any():
                bvs = self.bv[:, s].astype(np.int64)
                for m in range(M):
                    act &= self.mvalid[:, m] != 0
                    d = np.abs(self.mv[:, m].astype(np.int64) - bvs).max(1)
                    hit = act & (d < thr)
                    self.mf[hit, m] = 0
                    self.bf[hit, s] = 0
            hi = ok & (h > maxh)
            lo = ok & ~hi
            maxh[hi] = h[hi]
            i_hi = index[hi]
            self.mv[ar[hi], i_hi] = self.mv[hi, 0]
            self.mvalid[ar[hi], i_hi] = 1
            self.mf[ar[hi], i_hi] = self.mf[hi, 0]
            self.mc[ar[hi], i_hi] = self.mc[hi, 0]
            self.mv[hi, 0] = self.bv[hi, s]
            self.mvalid[hi, 0] = 1
            self.mf[hi, 0] = self.bf[hi, s]
            self.mc[hi, 0] = self.bh[hi, s]
            i_lo = index[lo]
            self.mv[ar[lo], i_lo] = self.bv[lo, s]
            self.mvalid[ar[lo], i_lo] = 1
            self.mf[ar[lo], i_lo] = self.bf[lo, s]
            self.mc[ar[lo], i_lo] = self.bh[lo, s]
            index[ok] += 1

    def apply(self, frame):
        """One frame [rows][cols][3] -> (mask [rows][cols], background [rows][cols][3]), apply + getBackgroundImage."""
        px = np.ascontiguousarray(frame).reshape(self.n, 3)
        self.prev_ts = self.ts
        self.ts = self.ts + 1000. / float(self.p["fps"])
        if self.sudden and not self.bg_reset:  # changeBg
            self.ns = int(self.ns / 3.)
            self.sp = int(self.sp / 2.)
            self.bfc, self.bg_reset = 0, True
        fg = np.zeros(self.n, np.uint8)
        if self.mvalid[0, 0]:
            fg = self.filter_fg(self.detect(px))
        # updateBg
        if self.bg_reset and self.bfc > (self.ns - 1) % (1 << 32):
            self.bfc = (self.ns - 1) % (1 << 32)
        if float(self.pbft) > self.ts:
            self.pbft = int(self.ts)
        if self.bfc == (self.ns - 1) % (1 << 32):
            self.create_bg(self.bfc, fg)
            self.bfc = 0
        elif self.ts - float(self.pbft) >= float(self.sp):
            self.pbft = int(self.ts)
            self.sample = px.copy()
            self.create_bg(self.bfc, fg)
            self.bfc += 1
        if not self.mvalid[0, 0]:
            return np.zeros((self.rows, self.cols), np.uint8), np.zeros((self.rows, self.cols, 3), np.uint8)
        return fg.reshape(self.rows, self.cols).copy(), self.bgimg.reshape(self.rows, self.cols, 3).copy()

    def control(self):
        return np.array([self.ts, self.prev_ts, self.pbft, self.bfc, self.ns, self.sp, self.bg_reset, self.sudden, self.M, self.mvalid[0, 0] != 0], np.float64)

    def planes(self):
        bins = np.concatenate([self.bv, self.bh[..., None], self.bf[..., None]], axis=2).astype(np.uint8)
        model = np.concatenate([self.mv, self.mvalid[..., None], self.mf[..., None], self.mc[..., None]], axis=2).astype(np.uint8)
        return {"bins": bins, "model": model, "persistence": self.persist.copy()}


def run(params, frames, area_filter=area_filter_follower):
    """masks [T][H][W], backgrounds [T][H][W][3], control [T][10], the model after the last frame."""
    T, H, W = frames.shape[:3]
    m = Model(params, H, W, area_filter)
    masks, bgs, ctl = np.zeros((T, H, W), np.uint8), np.zeros((T, H, W, 3), np.uint8), np.zeros((T, len(CONTROL)))
    for t in range(T):
        masks[t], bgs[t] = m.apply(frames[t])
        ctl[t] = m.control()
    return masks, bgs, ctl, m


# ------------------------------------------------------------------------------------------------------------------ clips and cases
def _noise(rng, shape, amp):
    return rng.integers(-amp, amp + 1, shape)


def clip(kind, T, H, W, seed):
    """Seeded clips.  Backgrounds stay inside 20..140 per channel and objects inside 170..250, so that no sample is within the
    association threshold of a byte pattern an uninitialised bin may hold in the reference (0xA5 = 165, 0x5A = 90 +- 5 are avoided
    by the background palette below) - see DESIGN.md §4."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([30 + (xx * 3 + yy) % 40, 100 + (yy * 2 + xx) % 30, 40 + (xx + yy * 3) % 35], axis=-1).astype(np.int64)
    out = np.zeros((T, H, W, 3), np.uint8)

    def put(img, y0, y1, x0, x1, colour):
        y0, y1, x0, x1 = max(y0, 0), min(y1, H), max(x0, 0), min(x1, W)
        if y0 < y1 and x0 < x1:
            img[y0:y1, x0:x1] = colour

    for t in range(T):
        img = base + _noise(rng, (H, W, 3), 1)
        if kind == "box":  # static scene + a box that moves one pixel a frame
            bh, bw = max(2, H // 3), max(2, W // 4)
            put(img, H // 4, H // 4 + bh, (t * 2) % max(W - bw, 1), (t * 2) % max(W - bw, 1) + bw, (200, 220, 240))
            put(img, H - 3, H - 2, 1 + t % max(W - 3, 1), 2 + t % max(W - 3, 1), (250, 180, 200))  # one-pixel speck: dropped by minArea
        elif kind == "late":  # nothing moves until the wrapper's defaults have built their first model (frame 145)
            if t >= 147:
                put(img, H // 4, H // 4 + 8, (t * 2) % max(W - 9, 1), (t * 2) % max(W - 9, 1) + 9, (200, 220, 240))
        elif kind == "persist":  # an object arrives after the first model and stays
            if t >= 8:
                put(img, H // 3, H // 3 + 6, W // 3, W // 3 + 8, (210, 200, 230))
            put(img, 2, 7, (t * 3) % (W - 6), (t * 3) % (W - 6) + 6, (180, 240, 190))
        elif kind == "shadow":
            if t >= T // 2:
                img[:, : W // 3] = img[:, : W // 3] * 8 // 10          # inside [alpha, beta)
                img[:, W // 3: 2 * W // 3] = img[:, W // 3: 2 * W // 3] * 4 // 10  # below alpha
                put(img, H - 6, H - 1, W - 8, W - 1, (90 + 60, 90 + 60, 90 + 60))  # gray on a coloured background
            put(img, 1, 5, 1, 6, (60, 60, 60))   # a gray background patch (hue through NaN)
            put(img, 6, 9, 1, 6, (0, 0, 0))      # v_b == 0
            if t >= T // 2:
                put(img, 1, 9, 1, 4, (20, 20, 20))
        elif kind == "holes":
            if t >= T // 2:
                c = (230, 210, 190)
                put(img, 2, 14, 2, 16, c)          # a ring ...
                put(img, 4, 12, 4, 14, base[4:12, 4:14])
                put(img, 6, 9, 6, 9, c)            # ... with a blob in its hole
                put(img, 7, 8, 7, 8, base[7:8, 7:8])  # ... that has a one-pixel hole itself
                put(img, 10, 11, 11, 12, c)        # a speck in the hole
                put(img, 0, 5, W - 6, W, c)        # a blob on the image frame
                put(img, H - 1, H, 3, 9, c)        # on the bottom frame row only
                put(img, 17, 20, 3, 6, c)          # a 3x3 blob: area 4
                put(img, 17, 19, 9, 11, c)         # 2x2: area 1
                put(img, 16, 22, 14, 20, c)        # a small ring whose hole is one pixel
                put(img, 18, 19, 16, 17, base[18:19, 16:17])
                put(img, 17, 18, 22, 23, c)        # diagonal pair
                put(img, 18, 19, 23, 24, c)
        elif kind == "bigring":  # a ring whose outer border is above 0.6 numPixels and whose hole border is below it
            if t >= T // 2:
                c = (230, 210, 190)
                put(img, 1, H - 1, 1, W - 1, c)
                put(img, 4, H - 4, 4, W - 4, base[4:H - 4, 4:W - 4])
                put(img, 8, 11, 8, 11, c)      # a blob in the hole
                put(img, 14, 15, 20, 21, c)    # a speck in the hole: kept with the hole's contour
        elif kind == "sudden":
            if t >= T // 3:
                put(img, 0, H, 0, (W * 3) // 4, (215, 235, 225))
        elif kind == "full":  # numSamples 10, minBinHeight 3: a block whose ten samples are a a b c e a b b c (c): bins 3 3 3 1
            put(img, 2, 6, 2, 6, (20 + 25 * [0, 0, 1, 2, 3, 0, 1, 1, 2, 2][t % 10], 100, 50))
            if t >= 10:  # after the first model
                put(img, 8, 13, (t * 2) % (W - 5), (t * 2) % (W - 5) + 5, (200, 220, 240))
        out[t] = np.clip(img, 0, 255).astype(np.uint8)
    return out


def frames_of(spec):
    kind, T, H, W, seed = spec.split(":")
    if kind == "file":  # the repository's own clip, first T frames
        z = np.load(os.path.join(GOLDEN, "frames_96x80.npz"))
        key = [k for k in z.files if z[k].ndim == 4][0]
        return np.ascontiguousarray(z[key][: int(T)])
    return clip(kind, int(T), int(H), int(W), int(seed))


FAST = dict(numSamples=6, fps=10.0, samplingPeriod=100)  # a sample every frame, a model every 6


def cases():
    """Ordered {case: params}: the constructor's values + `input` = "kind:T:H:W:seed" + optional `window`."""
    c = {}

    def add(name, inp, window=None, **kw):
        p = dict(DEFAULTS, input=inp, **kw)
        if window:
            p["window"] = list(window)
        c[name] = p

    add("default_short", "file:12:80:96:0")
    add("basic", "box:20:24:32:1", **FAST)
    add("tile", "box:20:16:64:2", **FAST)
    add("ragged", "box:22:37:53:3", (0, 20), **FAST)
    add("ragged_o1", "box:22:37:53:3", (1, 21), **FAST)
    add("ragged_o2", "box:22:37:53:3", (2, 22), **FAST)
    add("tiny1x1", "box:16:1:1:4", **FAST)
    add("tiny3x3", "box:16:3:3:5", **FAST)
    add("persist", "persist:40:20:30:6", numSamples=6, fps=30.0, samplingPeriod=33, persistencePeriod=120, minArea=4.0)
    add("shadow", "shadow:20:20:30:7", **FAST)
    add("holes_a0", "holes:16:24:30:8", minArea=0.0, **FAST)
    add("holes_a2", "holes:16:24:30:8", minArea=2.5, **FAST)
    add("holes_a30", "holes:16:24:30:8", minArea=30.0, **FAST)
    add("holes_big", "bigring:16:24:30:14", minArea=2.5, **FAST)
    add("sudden", "sudden:40:16:24:9", numSamples=10, fps=10.0, samplingPeriod=100)
    add("morph", "box:20:24:32:10", morphologicalFiltering=1, **FAST)
    add("minbin1", "box:20:16:24:11", minBinHeight=1, minArea=4.0, **FAST)
    add("minbin3", "box:20:16:24:12", minBinHeight=3, minArea=4.0, **FAST)
    add("full", "full:20:14:20:13", minArea=4.0, numSamples=10, minBinHeight=3, fps=10.0, samplingPeriod=100)
    return c


def case_frames(p):
    f = frames_of(p["input"])
    if "window" in p:
        f = f[p["window"][0]:p["window"][1]]
    return f


def load():
    """{case: dict(params, frames, masks [T][H][W], bg_crc [T], control [T][10], and for small cases bins / model / persistence)}"""
    z = np.load(os.path.join(GOLDEN, "imbs_ref.npz"))
    out = {}
    for name in json.loads(bytes(z["cases"]).decode()):
        p = json.loads(bytes(z[name + "/params"]).decode())
        frames = case_frames(p)
        assert crc(frames) == int(z[name + "/input_crc"]), name
        r = dict(params=p, frames=frames, masks=z[name + "/masks"], bg_crc=z[name + "/bg_crc"], control=z[name + "/control"])
        for pl in ("bins", "model", "persistence"):
            if name + "/" + pl in z.files:
                r[pl] = z[name + "/" + pl]
        out[name] = r
    return out
