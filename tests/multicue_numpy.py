"""numpy restatement of the model stage of SJN_MultiCueBGS (package_bgs/sjn/SJN_MultiCueBGS.cpp), vectorised over
the books: frame reduction, the 7 x 7 blur, the HSV-cone conversion, texture and colour codebooks with their cache-books, training,
confidence and landmark maps, the model update with absorption.  Books are fixed-capacity slot arrays like the device's; an insert
or absorption into a full book is dropped and counted in `overflow`.  `counts` holds how often each branch of COUNTERS was taken.
Pinned bit for bit to the reference's own code by tests/golden/multicue_ref.npz (tools/ref_fixtures/multicue)."""
import zlib

import numpy as np

FIELDS = ("training_period", "t_model_threshold", "c_model_threshold", "learning_rate", "texture_train_vol_range", "color_train_vol_range",
          "absorption_enable", "absorption_period", "reduced_width", "reduced_height", "back_clear_period", "cache_clear_period")
INT_FIELDS = tuple(k for k in FIELDS if k != "learning_rate")
DEFAULTS = dict(training_period=20, t_model_threshold=1, c_model_threshold=10, learning_rate=0.05, texture_train_vol_range=15, color_train_vol_range=20,
                absorption_enable=1, absorption_period=200, reduced_width=160, reduced_height=120, back_clear_period=300, cache_clear_period=30)
FAST = dict(training_period=4, absorption_period=3, back_clear_period=6)  # every period fires within 40 frames
T_SLOTS, TCACHE_SLOTS, C_SLOTS, CCACHE_SLOTS = 20, 16, 32, 16  # BGS_MULTICUE_*_SLOTS: at least twice the largest book the reference reaches (10, 7, 16, 7)
NEI = ((-2, 0), (-1, -2), (1, -2), (2, 0), (1, 2), (-1, 2))  # (dx, dy), T_SetNeighborDirection
TAPS = (0, 2, 53, 146, 53, 2, 0)  # lrintf(getGaussianKernel(7, 0.7, CV_32F) * 256)
PI = 3.14159
COUNTERS = ("t_new", "t_update", "t_two_match", "c_new", "c_update", "c_two_match",
            "clear_all_kept", "clear_none_kept", "clear_partial",
            "cache_new", "cache_match_referred", "cache_match_other",
            "cache_mnrl_reset", "cache_increment", "cache_clear_removes",
            "absorb_texture", "absorb_colour",
            "lm_255_confidence", "lm_125", "lm_255_colour", "lm_0_texture",
            "t_grows_past_6", "c_grows_past_10", "cache_grows_past_3")


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xffffffff


def gaussian_kernel_f32(n, sigma):
    """cv::getGaussianKernel(n, sigma, CV_32F) for sigma > 0"""
    x = np.arange(n, dtype=np.float64) - (n - 1) * 0.5
    k = np.exp((-0.5 / (sigma * sigma)) * x * x).astype(np.float32)
    s = 0.0
    for v in k:
        s += float(v)
    return (k.astype(np.float64) * (1.0 / s)).astype(np.float32)


def integer_taps(n=7, sigma=0.7):
    return tuple(int(v) for v in np.rint(gaussian_kernel_f32(n, sigma) * np.float32(256.0)).astype(np.int64))


def reflect101(p, n):
    p = np.asarray(p).copy()
    if n == 1:
        return np.zeros_like(p)
    while ((p < 0) | (p >= n)).any():
        p = np.where(p < 0, -p, p)
        p = np.where(p >= n, 2 * (n - 1) - p, p)
    return p


def reduce_frame(frame, rh, rw):
    """ReduceImageSize (:545): src = (int)(i * ((double)H / rh))"""
    H, W = frame.shape[:2]
    sy = (np.arange(rh, dtype=np.float64) * (np.float64(H) / np.float64(rh))).astype(np.int64)
    sx = (np.arange(rw, dtype=np.float64) * (np.float64(W) / np.float64(rw))).astype(np.int64)
    return frame[sy][:, sx]


def blur7(img, taps=TAPS):
    """cv::GaussianBlur(7 x 7) on 8-bit data: integer taps, exact row pass, (sum + 2^15) >> 16, BORDER_REFLECT_101"""
    H, W = img.shape[:2]
    k = np.asarray(taps, np.int64)
    src = img.astype(np.int64)
    xs = np.stack([reflect101(np.arange(W) + j - 3, W) for j in range(7)])
    ys = np.stack([reflect101(np.arange(H) + j - 3, H) for j in range(7)])
    row = sum(k[j] * src[:, xs[j]] for j in range(7))
    col = sum(k[j] * row[ys[j]] for j in range(7))
    return np.clip((col + (1 << 15)) >> 16, 0, 255).astype(np.uint8)


def xyz_of(bgr, cos=np.cos, sin=np.sin):
    """BGR2HSVxyz_Par (:568): double arithmetic, PI = 3.14159, (uchar) truncation.  bgr: uint8 [..., 3]"""
    b, g, r = (bgr[..., c].astype(np.float64) / 255 for c in range(3))
    mn, mx = np.minimum(np.minimum(r, g), b), np.maximum(np.maximum(r, g), b)
    v = mx
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(v == 0, 0.0, (mx - mn) / mx)
        hr = 60 * (g - b) / s
        hr = np.where(hr < 0, 360 + hr, hr)
        hg = 120 + 60 * (b - r) / s
        hb = 240 + 60 * (r - g) / s
    h = np.where(mx == r, hr, np.where(mx == g, hg, hb))
    h = np.where((v == 0) | (s == 0), 0.0, h)
    h = h * ((2 * PI) / 360)
    out = np.empty(bgr.shape, np.uint8)
    out[..., 0] = (v * s * cos(h) * 127.5 + 127.5).astype(np.uint8)
    out[..., 1] = (v * s * sin(h) * 127.5 + 127.5).astype(np.uint8)
    out[..., 2] = (v * 255).astype(np.uint8)
    return out


class Books:
    """nb books of `cap` slots; a codeword has nm means of `dtype` and MNRL, first, last."""

    def __init__(self, nb, cap, nm, dtype):
        self.nb, self.cap, self.nm = nb, cap, nm
        self.total, self.num = np.zeros(nb, np.int32), np.zeros(nb, np.int32)
        self.mean = np.zeros((nb, cap, nm), dtype)
        self.meta = np.zeros((nb, cap, 3), np.int32)
        self.idx = np.arange(cap)[None, :]

    def valid(self):
        return self.idx < self.num[:, None]

    def compact(self, rows, keep):
        """rows: bool [nb]; keep: bool [nb][cap].  The kept entries of those books move to the front in order."""
        r = np.nonzero(rows)[0]
        if not r.size:
            return
        order = np.argsort(~keep[r], axis=1, kind="stable")
        self.mean[r] = np.take_along_axis(self.mean[r], order[:, :, None], 1)
        self.meta[r] = np.take_along_axis(self.meta[r], order[:, :, None], 1)
        self.num[r] = keep[r].sum(1)


class Model:
    def __init__(self, params=None, slots=None):
        self.p = dict(DEFAULTS, **(params or {}))
        p = self.p
        self.rw, self.rh = int(p["reduced_width"]), int(p["reduced_height"])
        self.n = n = self.rw * self.rh
        ts, tcs, cs, ccs = slots or (T_SLOTS, TCACHE_SLOTS, C_SLOTS, CCACHE_SLOTS)
        self.tb, self.tc = Books(n * 6, ts, 1, np.float32), Books(n * 6, tcs, 1, np.float32)
        self.cb, self.cc = Books(n, cs, 3, np.float64), Books(n, ccs, 3, np.float64)
        self.tref, self.tcnt = np.full(n * 6, -1, np.int16), np.zeros(n * 6, np.int16)
        self.cref, self.ccnt = np.full(n, -1, np.int16), np.zeros(n, np.int16)
        self.count, self.overflow = 0, 0
        self.counts = dict.fromkeys(COUNTERS, 0)
        y, x = np.divmod(np.arange(n), self.rw)
        self.interior = (x >= 2) & (x < self.rw - 2) & (y >= 2) & (y < self.rh - 2)
        self.nei = np.stack([np.clip(y + dy, 0, self.rh - 1) * self.rw + np.clip(x + dx, 0, self.rw - 1) for dx, dy in NEI], 1)  # [n][6]; used on the interior only
        self.gauss = self.xyz = np.zeros((n, 3), np.uint8)
        self.conf, self.landmark = np.zeros(n, np.float32), np.zeros(n, np.uint8)
        self.have_landmark = False
        self.absorb = bool(p["absorption_enable"])
        self.rate = np.float32(p["learning_rate"])

    # ---- PreProcessing (:259)
    def preprocess(self, frame):
        red = reduce_frame(np.asarray(frame), self.rh, self.rw)
        self.gauss = blur7(red).reshape(self.n, 3)
        self.xyz = xyz_of(self.gauss)

    def tdiff(self):
        z = self.xyz[:, 2].astype(np.int32)
        return (z[:, None] - z[self.nei]).astype(np.float32).reshape(-1)  # [n * 6]

    # ---- T_ModelConstruction (:1320) / C_CodebookConstruction (:1804) on the books `act`
    def construct(self, bk, act, sample, rng, rate, background, ref, cnt, tag):
        c = self.counts
        v = bk.valid()
        if bk.nm == 1:
            m = (bk.mean[:, :, 0] - np.float32(rng) <= sample[:, None]) & (sample[:, None] <= bk.mean[:, :, 0] + np.float32(rng)) & v
        else:
            s = sample.astype(np.float64)[:, None, :]
            m = ((bk.mean - float(rng) <= s) & (s <= bk.mean + float(rng))).all(2) & v
        nm = m.sum(1)
        first = m.argmax(1)
        new, upd = act & (nm == 0), act & (nm > 0)
        bk.total[act] += 1
        full = new & (bk.num >= bk.cap)
        ins = new & ~full
        self.overflow += int(full.sum())
        r = np.nonzero(ins)[0]
        slot = bk.num[r]
        bk.mean[r, slot] = sample[r].reshape(len(r), bk.nm).astype(bk.mean.dtype)
        bk.meta[r, slot, 0], bk.meta[r, slot, 1], bk.meta[r, slot, 2] = bk.total[r] - 1, bk.total[r], bk.total[r]
        bk.num[r] += 1
        u = np.nonzero(upd)[0]
        f = first[u]
        neg = np.float32(1) - rate
        if bk.nm == 1:
            bk.mean[u, f, 0] = rate * sample[u] + neg * bk.mean[u, f, 0]
        else:
            bk.mean[u, f] = (rate * sample[u].astype(np.float32)).astype(np.float64) + np.float64(neg) * bk.mean[u, f]
        bk.meta[u, f, 2] = bk.total[u]
        if background:
            c[tag + "_new"] += int(new.sum()); c[tag + "_update"] += int(upd.sum()); c[tag + "_two_match"] += int((act & (nm >= 2)).sum())
            grown = int((ins & (bk.num > (6 if bk.nm == 1 else 10))).sum())
            c["t_grows_past_6" if bk.nm == 1 else "c_grows_past_10"] += grown
            v = bk.valid() & act[:, None]
            negt = bk.total[:, None] - bk.meta[:, :, 2] + bk.meta[:, :, 1] - 1
            bk.meta[:, :, 0] = np.where(v & (bk.meta[:, :, 0] < negt), negt, bk.meta[:, :, 0])
            if self.absorb:
                ref[act] = -1
        else:
            c["cache_new"] += int(new.sum())
            c["cache_grows_past_3"] += int((ins & (bk.num > 3)).sum())
            bk.meta[r, slot, 0] = 0
            ref[r], cnt[r] = (bk.num[r] - 1).astype(np.int16), 1
            ref[full], cnt[full] = -1, 0  # a dropped insert refers to nothing
            same = f == ref[u]
            c["cache_match_referred"] += int(same.sum()); c["cache_match_other"] += int((~same).sum())
            cnt[u] = np.where(same, cnt[u] + np.int16(1), np.int16(1)).astype(np.int16)
            ref[u] = f.astype(np.int16)

    # ---- T_/C_ClearNonEssentialEntries (:1423, :1901)
    def clear(self, bk, act, period):
        c = self.counts
        go = act & (bk.total >= period)
        v = bk.valid()
        keep = v & (bk.meta[:, :, 0] <= int(period * 0.5))
        kc = keep.sum(1)
        whole = go & ((kc == 0) | (kc == bk.num))
        part = go & ~whole
        c["clear_all_kept"] += int((go & (kc == bk.num) & (bk.num > 0)).sum()); c["clear_none_kept"] += int((go & (kc == 0) & (bk.num > 0)).sum()); c["clear_partial"] += int(part.sum())
        bk.compact(part, keep)
        w = bk.valid() & go[:, None]
        bk.meta[w] = (0, 1, 1)
        bk.total[go] = 0

    # ---- T_/C_ClearNonEssentialEntriesForCachebook (:1494, :1965): the literal period 10 and stale threshold 5
    def cache_clear(self, bk, act, lm255, ref):
        c = self.counts
        inc = act & (bk.total < 10)
        clr = act & ~inc
        v = bk.valid()
        hit = v & inc[:, None] & lm255[:, None] & (bk.idx == ref[:, None])
        up = v & inc[:, None] & ~hit
        c["cache_mnrl_reset"] += int(hit.sum()); c["cache_increment"] += int(up.sum())
        bk.meta[:, :, 0] = np.where(hit, 0, np.where(up, bk.meta[:, :, 0] + 1, bk.meta[:, :, 0]))
        bk.total[inc] += 1
        keep = v & (bk.meta[:, :, 0] < 5)
        c["cache_clear_removes"] += int((clr & (keep.sum(1) < bk.num)).sum())
        bk.compact(clr, keep)
        w = bk.valid() & clr[:, None]
        bk.meta[:, :, 0] = np.where(w, 0, bk.meta[:, :, 0])
        bk.total[clr] = 0

    # ---- T_/C_Absorption (:1612, :2025): the referred index and the count are left as they are
    def absorption(self, model, cache, act, ref, cnt, tag):
        go = act & (cnt >= self.p["absorption_period"])
        full = go & (model.num >= model.cap)
        self.overflow += int(full.sum())
        go &= ~full
        r = np.nonzero(go)[0]
        self.counts[tag] += len(r)
        if not len(r):
            return
        lv = ref[r].astype(np.int64)
        model.total[r] += 1
        slot = model.num[r]
        model.mean[r, slot] = cache.mean[r, lv]
        model.meta[r, slot, 0], model.meta[r, slot, 1], model.meta[r, slot, 2] = model.total[r] - 1, model.total[r], model.total[r]
        model.num[r] += 1
        keep = cache.valid() & (cache.idx != ref[:, None])
        cache.compact(go, keep)

    # ---- BackgroundModeling_Par (:274) with the counter of process (:85-88)
    def train(self, frame):
        p = self.p
        assert self.count <= p["training_period"], "training is complete"
        self.preprocess(frame)
        rate = self.rate * np.float32(4)
        a1, a6 = self.interior, np.repeat(self.interior, 6)
        self.construct(self.tb, a6, self.tdiff(), p["texture_train_vol_range"], rate, True, self.tref, self.tcnt, "t")
        self.construct(self.cb, a1, self.xyz, p["color_train_vol_range"], rate, True, self.cref, self.ccnt, "c")
        if self.count == p["training_period"]:
            self.clear(self.tb, a6, p["training_period"])
            self.clear(self.cb, a1, p["training_period"])
            self.count += 1
        self.count += 1

    # ---- PreProcessing, T_GetConfidenceMap_Par (:1567), CreateLandmarkArray_Par (:434)
    def landmark_map(self, frame):
        p, c = self.p, self.counts
        assert self.count > p["training_period"], "training is not complete"
        self.preprocess(frame)
        n, it = self.n, self.interior
        d = self.tdiff()
        tb = self.tb
        tr = np.float32(p["texture_train_vol_range"])
        mean = tb.mean[:, :, 0]
        m = ((mean - tr) - np.float32(5) <= d[:, None]) & (d[:, None] <= (mean + tr) + np.float32(5)) & tb.valid()
        matched = m.any(1).reshape(n, 6).sum(1)
        conf = np.float32(1) - matched.astype(np.float32) / np.float32(6)
        self.conf = np.where(it, conf, np.float32(0)).astype(np.float32)
        thr = np.float32(p["t_model_threshold"]) / np.float32(6)
        back, dcnt = np.zeros(n), np.zeros(n)
        tm, tv = mean.reshape(n, 6, tb.cap), tb.valid().reshape(n, 6, tb.cap)
        for k in range(6):
            for j in range(tb.cap):
                back = np.where(tv[:, k, j], back + tm[:, k, j].astype(np.float64), back)
                dcnt += tv[:, k, j]
        with np.errstate(divide="ignore", invalid="ignore"):
            back = back / dcnt
        inp = np.abs(d.astype(np.float64)).reshape(n, 6).sum(1)
        cr = float(p["color_train_vol_range"])
        s = self.xyz.astype(np.float64)[:, None, :]
        cm = (((self.cb.mean - cr - 10 <= s) & (s <= self.cb.mean + cr + 10)).all(2) & self.cb.valid()).any(1)
        by_conf = it & (self.conf > thr)
        flat = it & ~by_conf & (back < 50) & (inp < 50)
        lm = np.zeros(n, np.uint8)
        lm[by_conf] = 255
        lm[flat & cm] = 125
        lm[flat & ~cm] = 255
        c["lm_255_confidence"] += int(by_conf.sum()); c["lm_125"] += int((flat & cm).sum()); c["lm_255_colour"] += int((flat & ~cm).sum())
        c["lm_0_texture"] += int((it & ~by_conf & ~flat).sum())
        self.landmark = lm
        self.have_landmark = True
        return lm.reshape(self.rh, self.rw), self.conf.reshape(self.rh, self.rw)

    # ---- step 2 of EvaluateGhostRegion (:1029-1046) / of UpdateModel_Par (:384-427); the map's border is ignored
    def update(self, umap, ghost):
        p = self.p
        assert self.have_landmark, "no landmark call since the last update"
        on = np.asarray(umap).reshape(self.n) != 0
        bg1 = self.interior & on
        bg6 = np.repeat(bg1, 6)
        d = self.tdiff()
        tr, cr = p["texture_train_vol_range"], p["color_train_vol_range"]
        self.construct(self.tb, bg6, d, tr, self.rate, True, self.tref, self.tcnt, "t")
        self.construct(self.cb, bg1, self.xyz, cr, self.rate, True, self.cref, self.ccnt, "c")
        self.clear(self.tb, bg6, p["back_clear_period"])
        self.clear(self.cb, bg1, p["back_clear_period"])
        if ghost:
            return
        self.have_landmark = False
        if not self.absorb:
            return
        ca1 = self.interior & ~on
        ca6 = np.repeat(ca1, 6)
        self.construct(self.tc, ca6, d, tr, self.rate, False, self.tref, self.tcnt, "t")
        self.construct(self.cc, ca1, self.xyz, cr, self.rate, False, self.cref, self.ccnt, "c")
        self.absorption(self.tb, self.tc, ca6, self.tref, self.tcnt, "absorb_texture")
        self.absorption(self.cb, self.cc, ca1, self.cref, self.ccnt, "absorb_colour")
        lm1 = self.landmark == 255
        self.cache_clear(self.tc, np.repeat(self.interior, 6), np.repeat(lm1, 6), self.tref)
        self.cache_clear(self.cc, self.interior, lm1, self.cref)

    def state(self):
        """the planes of bgs_multicue_get_state, slots at and beyond m_iNumEntries 0"""
        n = self.n
        out = {"gauss": self.gauss, "xyz": self.xyz, "conf": self.conf, "landmark": self.landmark, "count": np.array([self.count], np.int64),
               "overflow": np.array([self.overflow], np.int64), "tref": self.tref.reshape(n, 6), "tcnt": self.tcnt.reshape(n, 6), "cref": self.cref, "ccnt": self.ccnt}
        for name, bk, shape in (("t", self.tb, (n, 6)), ("tcache", self.tc, (n, 6)), ("c", self.cb, (n,)), ("ccache", self.cc, (n,))):
            v = bk.valid()
            means = np.where(v[:, :, None], bk.mean, 0).astype(bk.mean.dtype)
            meta = np.where(v[:, :, None], bk.meta, 0).astype(np.int32)
            book = np.stack([bk.total, bk.num], 1)
            short = name in ("t", "c")
            out[name + "book" if short else name] = book.reshape(shape + (2,))
            out[name + "means" if short else name + "_means"] = means.reshape(shape + (bk.cap,)) if bk.nm == 1 else means.reshape(shape + (bk.cap, 3))
            out[name + "meta" if short else name + "_meta"] = meta.reshape(shape + (bk.cap, 3))
        return out


PLANES = ("gauss", "xyz", "conf", "landmark", "tbook", "tcache", "tmeans", "tcache_means", "tmeta", "tcache_meta", "tref", "tcnt",
          "cbook", "ccache", "cmeans", "ccache_means", "cmeta", "ccache_meta", "cref", "ccnt", "count", "overflow")


def run(params, frames, ghost_maps, update_maps, slots=None):
    """The fixture's call sequence: training_period + 1 training frames, then landmark / ghost update / update per frame.
    Returns (model, landmarks [D][rh][rw], confs [D][rh][rw])."""
    m = Model(params, slots)
    T0 = m.p["training_period"] + 1
    lms, confs = [], []
    for t, f in enumerate(frames):
        if t < T0:
            m.train(f)
            continue
        lm, cf = m.landmark_map(f)
        lms.append(lm.copy()), confs.append(cf.copy())
        m.update(ghost_maps[t - T0], True)
        m.update(update_maps[t - T0], False)
    return m, np.array(lms), np.array(confs)


STATE_PLANES = tuple(k for k in PLANES if k not in ("conf", "landmark", "count", "overflow"))  # the planes the fixture stores (as CRCs)
_FIXTURE = None


def load():
    """tests/golden/multicue_ref.npz as {case: record}.  The frames, ghost maps and boxes are made again by tests/multicue_scenes.py
    and the frames checked against the stored CRC; `update` is the g_aUpdateMap the reference built from the boxes."""
    global _FIXTURE
    if _FIXTURE is None:
        import os
        import multicue_scenes as sc
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multicue_ref.npz"))
        out = {"_counters": dict(zip((str(k) for k in z["counter_names"]), (int(v) for v in z["counters"]))), "_maxima": tuple(int(v) for v in z["maxima"])}
        for name in (str(c) for c in z["cases"]):
            p = {k: (int(v) if k in INT_FIELDS else float(v)) for k, v in zip(FIELDS, z[name + ".params"])}
            rows, cols, T, seed = (int(v) for v in z[name + ".geom"])
            gen, train = str(z[name + ".scene"][0]), p["training_period"] + 1
            frames = sc.frames_of(gen, rows, cols, T, train, seed)
            assert crc(frames) == int(z[name + ".frames_crc"][0]), name
            ghost, boxes = sc.maps_of(gen, p["reduced_height"], p["reduced_width"], T - train)
            r = {"params": p, "frames": frames, "ghost": ghost, "boxes": boxes, "train": train, "landmark": z[name + ".landmark"], "conf": z[name + ".conf"],
                 "update": z[name + ".update"], "count": int(z[name + ".count"][0]), "maxima": tuple(int(v) for v in z[name + ".maxima"]),
                 "plane_crc": dict(zip(STATE_PLANES, (int(v) for v in z[name + ".plane_crc"]))),
                 "planes": {k: z[name + "." + k] for k in STATE_PLANES if name + "." + k in z.files}}
            for a in (frames, ghost, boxes):
                a.setflags(write=False)
            out[name] = r
        _FIXTURE = out
    return _FIXTURE


def cases():
    return [k for k in load() if not k.startswith("_")]
