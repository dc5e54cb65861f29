"""numpy restatement of package_bgs/jmo's MultiLayerBGS (Yao and Odobez: LBP + colour layers) as the engine's BGS_MULTILAYER class
computes it, with branch counters.  Vectorised over pixels; every float operation is float32 in the reference's order
(CMultiLayerBGS.cpp:375-801, :1485-1610, LocalBinaryPattern.cpp:124-309, the wrapper MultiLayerBGS.cpp:60-249).  expf is
float32(exp(float64)), the correctly rounded value: numpy's float32 exp is not.  DESIGN.md 5.11 lists the quirks kept here."""
import zlib

import numpy as np

F = np.float32
K = 5  # MAX_LBP_MODE_NUM: the slots the reference allocates before it learns max_mode_num
PI = F(3.141592653589793)
OFFS = ((2, 0), (1, -2), (-1, -2), (-2, 0), (-1, 2), (1, 2))  # CalNeigPixelOffset(2.0, 6, i): (x, y)
LBP_NOISE = F(6.0)  # ROBUST_COLOR_OFFSET: Init runs before the wrapper assigns robust_LBP_constant
MIN_SINE = np.sin(F(3.0) / F(180.0) * PI, dtype=F)  # sinf(3 degrees), the constructor's; overridden by the fixture's bits in the tests
P09 = F(1.0) - F(0.1)  # m_f1_MinLBPBinaryProb
COLOR_W = F(1.0) - F(0.5)  # m_fColorWeight, fixed by the constructor
RELIABLE = F(0.9)
MIN_LAYER_W = F(0.0001)

DEFAULTS = dict(max_mode_num=5, weight_updating_constant=5.0, texture_weight=0.5, bg_mode_percent=0.6, pattern_neig_half_size=4,
                pattern_neig_gaus_sigma=3.0, bg_prob_threshold=0.2, bg_prob_updating_threshold=0.2, robust_LBP_constant=3,
                min_noised_angle=float(F(10.0 / 180.0 * float(PI))), shadow_rate=0.6, highlight_rate=1.2, frame_duration=0.1,
                learn_mode_learn_rate_per_second=0.5, learn_weight_learn_rate_per_second=0.5, learn_init_mode_weight=0.05,
                detect_mode_learn_rate_per_second=0.01, detect_weight_learn_rate_per_second=0.01, detect_init_mode_weight=0.001,
                status=0, disable_detect_mode=1, disable_learning=0, detect_after=0)
FAST = dict(learn_weight_learn_rate_per_second=5.0, learn_mode_learn_rate_per_second=5.0, frame_duration=0.1, weight_updating_constant=0.0)
FIELDS = list(DEFAULTS)  # the order of bgs_multilayer_params after struct_size
INT_FIELDS = ("max_mode_num", "pattern_neig_half_size", "robust_LBP_constant", "status", "disable_detect_mode", "disable_learning", "detect_after")
COUNTERS = ("add", "replace", "match", "layer_created", "removal_first", "removal_second", "stale_decay_matched", "penalty", "range_one", "norm_zero", "ratio_ge_one")


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xffffffff


def expf(x):
    return np.exp(x.astype(np.float64)).astype(F)


def gaussian_kernel(n, sigma):
    """cv::getGaussianKernel(n, sigma, CV_32F), sigma > 0."""
    x = np.arange(n, dtype=np.float64) - (n - 1) * 0.5
    k = np.exp(-0.5 / (float(sigma) * float(sigma)) * x * x).astype(F)
    s = 0.0
    for v in k:
        s += float(v)
    return (k.astype(np.float64) * (1.0 / s)).astype(F)


def smooth(img, h, sigma):
    """cvSmooth(CV_GAUSSIAN, 2h+1, 2h+1, sigma) on a float plane, replicate border, in the summation order of the contract."""
    if h <= 0:
        return img.copy()
    k = gaussian_kernel(2 * h + 1, sigma)
    H, W = img.shape
    xs = np.clip(np.arange(W)[:, None] - h + np.arange(2 * h + 1)[None, :], 0, W - 1)
    row = k[0] * img[:, xs[:, 0]]
    for i in range(1, 2 * h + 1):
        row = row + k[i] * img[:, xs[:, i]]
    out = k[h] * row
    ys = np.arange(H)
    for i in range(1, h + 1):
        out = out + k[h + i] * (row[np.minimum(ys + i, H - 1)] + row[np.maximum(ys - i, 0)])
    return out.astype(F)


def gray(frame):
    f = frame.astype(np.int64)
    return ((f[..., 0] * 1868 + f[..., 1] * 9617 + f[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def lbp_bits(g):
    H, W = g.shape
    pad = np.zeros((H + 4, W + 4), F)
    pad[2:-2, 2:-2] = g
    c = g.astype(F)
    return np.stack([((c - pad[2 + oy:2 + oy + H, 2 + ox:2 + ox + W]) + LBP_NOISE > 0).astype(F) for ox, oy in OFFS], -1).reshape(H * W, 6)


def _quicksort(data, idx, low, high, ascent):
    """CMultiLayerBGS::QuickSort, literally."""
    i, j = low, high
    z = data[(low + high) // 2]
    while True:
        if ascent:
            while data[i] < z:
                i += 1
            while data[j] > z:
                j -= 1
        else:
            while data[i] > z:
                i += 1
            while data[j] < z:
                j -= 1
        if i <= j:
            data[i], data[j] = data[j], data[i]
            idx[i], idx[j] = idx[j], idx[i]
            i += 1
            j -= 1
        if not i <= j:
            break
    if low < j:
        _quicksort(data, idx, low, j, ascent)
    if i < high:
        _quicksort(data, idx, i, high, ascent)


_perm_cache = {}


def sort_desc(wr, idx, cnt):
    """QuickSort(weights, lbp_idxes, 0, cnt - 1, false) per row.  wr[n, K] are the weights in list order.  What the sort does depends
    on the outcomes of its comparisons only, so rows are grouped by the order pattern of their weights and the literal sort runs once
    per pattern."""
    n = len(cnt)
    code = cnt.astype(np.int64).copy()
    m = 8
    for i in range(K):
        for j in range(i + 1, K):
            both = (i < cnt) & (j < cnt)
            code += m * np.where(both, np.sign(wr[:, i] - wr[:, j]).astype(np.int64) + 1, 1)
            m *= 3
    out = idx.copy()
    for c in np.unique(code[cnt > 1]):
        rows = np.nonzero((code == c) & (cnt > 1))[0]
        if c not in _perm_cache:
            r = rows[0]
            k = int(cnt[r])
            d, p = [float(v) for v in wr[r, :k]], list(range(k))
            _quicksort(d, p, 0, k - 1, False)
            _perm_cache[c] = p
        p = _perm_cache[c]
        out[rows[:, None], np.arange(len(p))[None, :]] = idx[rows[:, None], np.array(p)[None, :]]
    return out


class Model:
    def __init__(self, params, rows, cols, min_sine_bits=None):
        p = dict(DEFAULTS, **params)
        self.p, self.rows, self.cols = p, rows, cols
        n = self.n = rows * cols
        self.num, self.bgn, self.idx = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros((n, K), np.int64)
        self.pat, self.bg, self.mx, self.mn = np.zeros((n, K, 6), F), np.zeros((n, K, 3), F), np.zeros((n, K, 3), F), np.zeros((n, K, 3), F)
        self.w, self.mw, self.lay = np.zeros((n, K), F), np.zeros((n, K), F), np.zeros((n, K), np.int64)
        self.dist = np.zeros((rows, cols), F)
        self.frame_no = 0
        self.counts = dict.fromkeys(COUNTERS, 0)
        self.min_sine = MIN_SINE if min_sine_bits is None else np.array([min_sine_bits], np.uint32).view(F)[0]
        self.min_angle = F(p["min_noised_angle"])
        self.status = 0 if p["disable_detect_mode"] else int(p["status"])
        self.learning_disabled = bool(p["disable_learning"]) if self.status == 1 else False
        fd = F(p["frame_duration"])
        pre = "learn" if self.status == 0 else "detect"
        self._set_rates(F(p[pre + "_mode_learn_rate_per_second"]), F(p[pre + "_weight_learn_rate_per_second"]), F(p[pre + "_init_mode_weight"]))
        self.fd = fd

    def _set_rates(self, mode, weight, init):  # SetParameters
        fd = F(self.p["frame_duration"])
        self.mrate, self.wrate, self.init_w = F(mode * fd), F(weight * fd), F(init)
        self.m1 = F(1.0) - self.mrate

    def constants_bits(self):
        return int(np.array([self.min_sine], F).view(np.uint32)[0]), int(np.array([self.min_angle], F).view(np.uint32)[0])

    def _listed(self):
        a = np.arange(K)[None, :]
        ls = np.zeros((self.n, K), bool)
        for r in range(K):
            ls[np.arange(self.n), self.idx[:, r]] |= r < self.num
        del a
        return ls

    def _rerank(self, rows_mask):
        """the tail of RemoveBackgroundLayers and of the pixel loop: sort the list by weight, then bg_num"""
        ar = np.arange(self.n)
        wr = np.take_along_axis(self.w, self.idx, 1)
        tot = np.zeros(self.n, F)
        for a in range(K):
            tot = np.where(a < self.num, tot + wr[:, a], tot)
        new = sort_desc(wr, self.idx, np.where(rows_mask, self.num, 0))
        self.idx = np.where(rows_mask[:, None], new, self.idx)
        thr = F(self.p["bg_mode_percent"]) * tot
        wr = np.take_along_axis(self.w, self.idx, 1)
        cum, found = np.zeros(self.n, F), np.full(self.n, -1)
        for a in range(K):
            cum = np.where(a < self.num, cum + wr[:, a], cum)
            found = np.where((found < 0) & (a < self.num) & (cum > thr), a + 1, found)
        del ar
        return found  # -1: no prefix exceeds

    def _renumber_layers(self, rows_mask):
        """the layer renumbering at the end of RemoveBackgroundLayers: an ascending QuickSort of distinct layer numbers = their rank"""
        ls = self._listed() & (self.lay > 0)
        lay = np.where(ls, self.lay, 0)
        for s in range(K):
            for t in range(s + 1, K):
                assert not np.any(ls[:, s] & ls[:, t] & (lay[:, s] == lay[:, t])), "layer numbers are distinct"
        rank = 1 + (ls[:, None, :] & (lay[:, None, :] < lay[:, :, None])).sum(-1)
        self.lay = np.where(rows_mask[:, None] & ls, rank, self.lay)

    def _remove_ranks(self, rem):
        """drop the listed ranks rem[n, K] from lbp_idxes, keeping the order"""
        keep = ~rem & (np.arange(K)[None, :] < self.num[:, None])
        order = np.argsort(~keep, axis=1, kind="stable")
        self.idx = np.take_along_axis(self.idx, order, 1)
        self.num = keep.sum(1)

    def apply(self, frame):
        p, n, ar = self.p, self.n, np.arange(self.n)
        C = self.counts
        if p["detect_after"] > 0 and p["detect_after"] == self.frame_no:  # MultiLayerBGS.cpp:200-218
            self.status = 1
            self._set_rates(F(0.01), F(0.01), F(0.001))
            self.learning_disabled = bool(p["disable_learning"])
        self.frame_no += 1
        learn = not self.learning_disabled
        tw = F(p["texture_weight"])
        cur = frame.reshape(n, 3).astype(F)
        cp = lbp_bits(gray(frame)) if tw > 0 else np.zeros((n, 6), F)
        wrate, wc = self.wrate, F(p["weight_updating_constant"])

        if learn:  # RemoveBackgroundLayers(PLBP): the first layered mode whose weight fell below 1e-4
            layr, wr = np.take_along_axis(self.lay, self.idx, 1), np.take_along_axis(self.w, self.idx, 1)
            cand = (layr != 0) & (wr < MIN_LAYER_W) & (np.arange(K)[None, :] < self.num[:, None])
            has = cand.any(1)
            first = np.argmax(cand, 1)
            rem = np.zeros((n, K), bool)
            rem[ar[has], first[has]] = True
            removed_layer = np.where(has, layr[ar, first], 0)
            C["removal_first"] += int(has.sum())
            self._remove_ranks(rem)
            ls = self._listed()
            self.lay = np.where(has[:, None] & ls & (self.lay > removed_layer[:, None]), self.lay - 1, self.lay)
            found = self._rerank(has)
            self.bgn = np.where(has, np.maximum(found, 0), self.bgn)
            self._renumber_layers(np.ones(n, bool))

        first_px = self.num == 0
        first_frame = bool(first_px[-1])  # bFirstFrame as the loop leaves it
        old = ~first_px
        raw = np.zeros(n, F)

        # find the best match, in rank order
        best, best_d = np.full(n, -1), np.full(n, F(999.0))
        offset = max(F(p["robust_LBP_constant"]), F(5.0))
        shadow, high = F(p["shadow_rate"]), F(p["highlight_rate"])
        for a in range(K):
            act = old & (a < self.num)
            s = self.idx[:, a]
            bg, mx, mn, pat = self.bg[ar, s], self.mx[ar, s], self.mn[ar, s], self.pat[ar, s]
            pd = (np.abs(cp - pat) > P09).sum(1).astype(F) / F(6.0) if tw > 0 else np.zeros(n, F)
            minI, maxI = np.minimum(mn, bg * shadow - F(5.0)), np.maximum(mx, bg * high + F(5.0))
            out = ((cur > maxI) | (cur < minI)).any(1)
            dot = n1 = n2 = np.zeros(n, F)
            for c in range(3):
                dot, n1, n2 = dot + bg[:, c] * cur[:, c], n1 + bg[:, c] * bg[:, c], n2 + cur[:, c] * cur[:, c]
            nn = n1 * n2
            with np.errstate(divide="ignore", invalid="ignore"):
                org = np.where(nn == 0, F(0), np.sqrt(np.maximum(F(1.0) - dot * dot / nn, F(0))))
                norm = np.sqrt(n1)
                sin_a = offset / norm
            noised = np.where(norm == 0, PI, np.where(sin_a < self.min_sine, self.min_angle, np.where(sin_a >= 1, PI, sin_a))).astype(F)
            ang = np.maximum(org - noised, F(0)).astype(F)
            cd = np.where(out, F(1.0), F(1.0) - expf(F(-100.0) * ang * ang)).astype(F)
            d = (COLOR_W * cd + tw * pd).astype(F)
            C["range_one"] += int((act & out).sum())
            C["norm_zero"] += int((act & ~out & (norm == 0)).sum())
            C["ratio_ge_one"] += int((act & ~out & (norm != 0) & ~(sin_a < self.min_sine) & (sin_a >= 1)).sum())
            better = act & (d < best_d)
            best, best_d = np.where(better, a, best), np.where(better, d, best_d).astype(F)

        bgn0 = self.bgn.copy()
        updating = best_d < F(p["bg_prob_updating_threshold"])
        ms = self.idx[ar, np.maximum(best, 0)]  # the matched slot
        pen = old & (best >= bgn0) & (self.mw[ar, ms] < RELIABLE)
        C["penalty"] += int(pen.sum())
        raw = np.where(old, np.where(pen, np.maximum(best_d, F(p["bg_prob_threshold"]) * F(2.5)), best_d), F(0)).astype(F)

        # the empty list: a first mode in slot 0, whether learning is disabled or not
        if first_px.any():
            self.pat[first_px, 0], self.bg[first_px, 0], self.mx[first_px, 0], self.mn[first_px, 0] = cp[first_px], cur[first_px], cur[first_px], cur[first_px]
            self.lay[first_px, 0], self.w[first_px, 0], self.mw[first_px, 0] = 0, self.init_w, self.init_w
            self.idx[first_px, 0], self.num[first_px], self.bgn[first_px] = 0, 1, 1
        if learn:
            nomatch, match = old & ~updating, old & updating
            decay = (F(1.0) - wrate / (F(1.0) + wc * self.mw)).astype(F)
            ls = self._listed()
            # no match: decay everything, then add or replace
            self.w = np.where(nomatch[:, None] & ls, self.w * decay, self.w).astype(F)
            add = nomatch & (self.num < p["max_mode_num"])
            rep = nomatch & ~add
            C["add"] += int(add.sum())
            C["replace"] += int(rep.sum())
            free = np.argmax(~ls[:, :p["max_mode_num"]], 1)
            tgt = np.where(add, free, self.idx[ar, p["max_mode_num"] - 1])
            r = np.nonzero(nomatch)[0]
            t = tgt[r]
            self.pat[r, t], self.bg[r, t], self.mx[r, t], self.mn[r, t] = cp[r], cur[r], cur[r], cur[r]
            self.lay[r, t], self.w[r, t], self.mw[r, t] = 0, self.init_w, self.init_w
            ra = np.nonzero(add)[0]
            self.idx[ra, self.num[ra]] = free[ra]
            self.num[ra] += 1
            # match
            C["match"] += int(match.sum())
            r = np.nonzero(match)[0]
            t = ms[r]
            self.bg[r, t] = self.m1 * self.bg[r, t] + self.mrate * cur[r]
            self.mn[r, t], self.mx[r, t] = np.minimum(cur[r], self.mn[r, t]), np.maximum(cur[r], self.mx[r, t])
            if tw > 0:
                self.pat[r, t] = self.m1 * self.pat[r, t] + self.mrate * cp[r]
            inc = (wrate * (F(1.0) + wc * self.mw[r, t])).astype(F)
            self.w[r, t] = (F(1.0) - inc) * self.w[r, t] + inc
            self.mw[r, t] = np.maximum(self.w[r, t], self.mw[r, t])
            mlay = np.where(match, self.lay[ar, ms], 0)
            # a layered match removes the higher layers that have decayed
            layr, wr, mwr = np.take_along_axis(self.lay, self.idx, 1), np.take_along_axis(self.w, self.idx, 1), np.take_along_axis(self.mw, self.idx, 1)
            ok = match & (mlay > 0) & (self.w[ar, ms] > self.mw[ar, ms] * F(0.2))
            rem = ok[:, None] & (np.arange(K)[None, :] < self.num[:, None]) & (layr > mlay[:, None]) & (wr < mwr * F(0.9))
            second = rem.any(1)
            C["removal_second"] += int(second.sum())
            if second.any():
                self._remove_ranks(rem)
                ls2 = self._listed()
                for b in range(K):  # the decrements in the order of removed_bg_layer_nums, each against the running value
                    self.lay = np.where((rem[:, b])[:, None] & ls2 & (self.lay > layr[:, b][:, None]), self.lay - 1, self.lay)
                found = self._rerank(second)
                self.bgn = np.where(second, np.maximum(found, 0), self.bgn)
                self._renumber_layers(second)
                newrank = np.argmax(self.idx == ms[:, None], 1)
                C["stale_decay_matched"] += int((second & (newrank != best)).sum())
            # or the matched mode becomes a layer
            create = match & (mlay == 0) & (self.mw[ar, ms] > RELIABLE)
            C["layer_created"] += int(create.sum())
            top = np.where(self._listed(), self.lay, 0).max(1)
            r = np.nonzero(create)[0]
            self.lay[r, ms[r]] = top[r] + 1
            # decay the others: by list position against the (possibly stale) best_match_idx
            decay = (F(1.0) - wrate / (F(1.0) + wc * self.mw)).astype(F)
            for a in range(K):
                act = match & (a < self.num) & (a != best)
                r = np.nonzero(act)[0]
                t = self.idx[r, a]
                self.w[r, t] = self.w[r, t] * decay[r, t]
            # sort the list by weight
            again = old & (self.num > 1)
            found = self._rerank(again)
            self.bgn = np.where(again, np.where(found > 0, found, bgn0), self.bgn)

        if first_frame:
            mask = np.zeros((self.rows, self.cols), np.uint8)
            self.dist = np.zeros((self.rows, self.cols), F)
        else:
            d = raw.reshape(self.rows, self.cols)
            h = int(p["pattern_neig_half_size"])
            self.dist = smooth(d, h, p["pattern_neig_gaus_sigma"]) if h >= 0 else d.copy()
            mask = np.where(self.dist > F(p["bg_prob_threshold"]), 255, 0).astype(np.uint8)
        top = self.bg[ar, self.idx[:, 0]]
        bgimg = np.where((self.num == 0)[:, None], 0, np.rint(top)).astype(np.uint8).reshape(self.rows, self.cols, 3)
        return mask, bgimg

    def state(self):
        """the bgs_get_state planes: order u8 [n][7], modes f32 [n][5][18], dist f32 [n]"""
        n = self.n
        order = np.zeros((n, 7), np.uint8)
        order[:, 0], order[:, 1] = self.num, self.bgn
        order[:, 2:] = np.where(np.arange(K)[None, :] < self.num[:, None], self.idx, 0)
        modes = np.concatenate([self.pat, self.bg, self.mx, self.mn, self.w[..., None], self.mw[..., None], self.lay[..., None].astype(F)], -1).astype(F)
        modes = np.where(self._listed()[..., None], modes, F(0))
        return order, modes, self.dist.reshape(n).copy()


def run(params, frames, min_sine_bits=None):
    m = Model(params, frames.shape[1], frames.shape[2], min_sine_bits)
    masks, bgs = [], []
    for f in frames:
        a, b = m.apply(f)
        masks.append(a), bgs.append(b)
    return m, np.stack(masks), np.stack(bgs)


CLASS_NAME = "MultiLayerBGS"
_fixture = None


def load():
    """tests/golden/multilayer_ref.npz as {case: record}; the frames come from tests/multilayer_scenes.py and are checked by CRC."""
    global _fixture
    if _fixture is None:
        import os

        import multilayer_scenes as sc
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multilayer_ref.npz"))
        out = {}
        for name in z["cases"]:
            name = str(name)
            rows, cols, T, seed = (int(v) for v in z[name + ".geom"])
            frames = sc.frames_of(z[name + ".scene"][0], rows, cols, T, seed)
            assert crc(frames) == int(z[name + ".frames_crc"][0]), name
            frames.setflags(write=False)
            vals = z[name + ".params"]
            params = {k: (int(v) if k in INT_FIELDS else float(v)) for k, v in zip(FIELDS, vals)}
            r = dict(params=params, frames=frames, masks=z[name + ".masks"], bg_crc=z[name + ".bg_crc"], order=z[name + ".order"], modes_crc=int(z[name + ".modes_crc"][0]),
                     dist=z[name + ".dist"], consts=z[name + ".consts"], expf=z[name + ".expf"])
            if name + ".modes" in z.files:
                r["modes"] = z[name + ".modes"]
            out[name] = r
        _fixture = out
    return _fixture


def cases():
    return list(load())
