"""float32 numpy restatement of package_bgs/tb FuzzySugenoIntegral / FuzzyChoquetIntegral (USTC_BGS types 21 and 22) on the RGB path
(colorSpace 1), written from FuzzyChoquetIntegral.cpp:31-173, FuzzyUtils.cpp and PixelUtils.cpp.  It reproduces
tests/golden/fuzzy_ref.npz bit for bit (tests/test_fuzzy_cpu.py) and is what the GPU tests compare the engine with on frames the
fixture does not hold.

The reference's Indice array is set once per frame and permuted further at every pixel, column by column, so the integral of a
pixel depends on every pixel before it.  Here that state is a prefix product over S3 computed by doubling (Hillis-Steele), not the
reference's serial loop: an independent statement of the scan the kernels run.
"""
import numpy as np

f32 = np.float32
SUGENO, CHOQUET = 1, 0
DEFAULTS = dict(ftl=10, alphaLearn=0.1, alphaUpdate=0.01, option=2, smooth=1, threshold=0.67)
_W = (1, 2, 4, 8, 0, 16, 32, 64, 128)  # CarreExp, FuzzyUtils.cpp:37-45 (slot 4 is the centre)


def lbp_table():
    """The 256 values the interior LBP can take: v = fl32(v + (bit_l * 2^l) / 255.0) over the nine slots, the term a double."""
    tab = np.zeros(256, f32)
    for code in range(256):
        v = f32(0)
        for l in range(9):
            bit = 1.0 if l == 4 else float((code >> (l if l < 4 else l - 1)) & 1)
            v = f32(float(v) + (bit * _W[l]) / 255.0)
        tab[code] = v
    return tab


_TAB = lbp_table()


def gray(img):  # float cvtColor(BGR2GRAY)
    return (img[..., 0] * f32(0.114) + img[..., 1] * f32(0.587)) + img[..., 2] * f32(0.299)


def _code(slots, centre):
    code = np.zeros(np.shape(centre), np.int64)
    for l, s in enumerate(slots):
        if l != 4:
            code += (s >= centre).astype(np.int64) * _W[l]
    return code


def lbp_plain(g):
    """The interior formula at every interior pixel (what the reference would compute without getNeighberhoodGrayPixel's quirk)."""
    H, W = g.shape
    out = np.zeros((H, W), f32)
    if H >= 3 and W >= 3:
        slots = [g[b:H - 2 + b, 2 - a:W - a] for a in range(3) for b in range(3)]  # slot 3a+b: column x+1-a, row y-1+b
        out[1:-1, 1:-1] = _TAB[_code(slots, g[1:-1, 1:-1])]
    return out


def lbp(g):
    """FuzzyUtils::LBP as it runs (x = y = 0 on entry): the corner (0,0), the interior, every other border pixel 0.
    getNeighberhoodGrayPixel compares the column with `height` and the row with `width`: in a frame with W >= H + 2 the interior pixels
    of column H take the `last line` branch (six slots refilled, three stale from the call before: the neighbourhood of column H-1),
    in a frame with H >= W + 2 those of row W take the `last column` branch (six slots in another order; the stale three are column
    W-3, rows W-2..W, left by the last full call, pixel (W-2, W-1))."""
    H, W = g.shape
    out = lbp_plain(g)
    c = g[0, 0]
    k = 2 * int(g[1, 0] >= c) + 4 * int(g[0, 1] >= c) + 8 * int(g[1, 1] >= c)
    out[0, 0] = f32(k / 255.0)
    if W >= H + 2 and H >= 3:
        out[1:-1, H] = out[1:-1, H - 1]
    if H >= W + 2 and W >= 3:
        y = W
        xs = np.arange(1, W - 1)
        slots = [g[y - 1, xs + 1], g[y, xs + 1], g[y - 1, xs], g[y, xs], g[y - 1, xs - 1], g[y, xs - 1],
                 np.full(xs.shape, g[W - 2, W - 3]), np.full(xs.shape, g[W - 1, W - 3]), np.full(xs.shape, g[W, W - 3])]
        out[y, 1:-1] = _TAB[_code(slots, slots[4])]
    return out


def ratio(c, b):
    """RatioPixels: min/max of the pair, 1 when equal.  For an unordered pair (a NaN background) the reference writes nothing and the
    integral reads uninitialised heap; the restatement and the engine give NaN."""
    with np.errstate(all="ignore"):
        return np.where(c < b, c / b, np.where(c > b, b / c, np.where(c == b, f32(1), f32(np.nan)))).astype(f32)


def sort3(h):
    """Trier on (n,3) values: three compare-exchanges with strict <, descending; returns the sorted values and the permutation pi with
    Indice_new[k] = Indice_old[pi[k]]."""
    h = h.copy()
    pi = np.tile(np.arange(3), (h.shape[0], 1))
    for a, b in ((1, 2), (0, 1), (1, 2)):
        sw = h[:, a] < h[:, b]
        h[sw, a], h[sw, b] = h[sw, b], h[sw, a]
        pi[sw, a], pi[sw, b] = pi[sw, b], pi[sw, a]
    return h, pi


def prefix_perm(pi):
    """sigma_q = pi_0 o pi_1 o ... o pi_q with (A o B)[k] = A[B[k]], by doubling."""
    s = pi.copy()
    d = 1
    while d < s.shape[0]:
        s[d:] = np.take_along_axis(s[:-d], s[d:], axis=1)
        d *= 2
    return s


def _mm(a, b):  # OpenCV's float median exchange: a = std::min(a, b), b = std::max(a, b)
    return np.where(b < a, b, a), np.where(a < b, b, a)


def median3(img):
    H, W = img.shape
    pd = np.pad(img, 1, mode="edge")
    p = [pd[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)]
    for i, j in ((1, 2), (4, 5), (7, 8), (0, 1), (3, 4), (6, 7), (1, 2), (4, 5), (7, 8), (0, 3), (5, 8), (4, 7), (3, 6), (1, 4), (2, 5), (4, 7), (4, 2), (6, 4), (4, 2)):
        p[i], p[j] = _mm(p[i], p[j])
    return p[4].astype(f32)


def to_u8(v):  # 32F -> 8U: round half to even, saturate, NaN -> 0
    with np.errstate(all="ignore"):
        return np.clip(np.rint(np.nan_to_num(v, nan=0.0)), 0, 255).astype(np.uint8)


class Fuzzy:
    def __init__(self, kind, identity_indice=False, **params):
        self.kind = kind
        self.p = dict(DEFAULTS)
        self.p.update(params)
        self.bg = None
        self.frame_number = 0
        self.integral = self.lbp_in = self.lbp_bg = None
        self.identity_indice = identity_indice  # coverage tests only: what a per-pixel Indice = (0,1,2) would give

    def process(self, frame, **params):
        """One frame (H,W,3 uint8).  Returns (mask, background bytes), both None while learning."""
        self.p.update(params)
        p = self.p
        inp = frame.astype(f32) * f32(1.0 / 255.0) + f32(0)
        out = (None, None)
        if self.frame_number <= p["ftl"]:
            if self.bg is None:
                self.bg = inp.copy()
            else:
                self.bg = (inp * f32(p["alphaLearn"]) + self.bg * f32(1 - p["alphaLearn"])) + f32(0)
        else:
            out = self._detect(inp)
        self.frame_number += 1
        return out

    def _detect(self, inp):
        p, bg = self.p, self.bg
        H, W = inp.shape[:2]
        self.lbp_in, self.lbp_bg = lbp(gray(inp)), lbp(gray(bg))
        tex = ratio(self.lbp_in, self.lbp_bg)
        col = ratio(inp, bg)
        if p["option"] == 1:
            G = np.array([0.4, 0.3, 0.3], f32)
        elif p["option"] == 2:
            G = np.array([0.6, 0.3, 0.1], f32)
        else:
            raise ValueError("option outside {1,2}: the reference's integral image is uninitialised memory")
        # column-major: q = x * H + y
        T = lambda a: np.ascontiguousarray(a.T).reshape(-1)
        if self.kind == CHOQUET and p["option"] == 1:
            hi = np.stack([T(col[..., 0]), T(col[..., 1]), T(col[..., 2])], 1)
        else:
            hi = np.stack([T(tex), T(col[..., 0]), T(col[..., 1])], 1)
        hs, pi = sort3(hi)
        sg = pi if self.identity_indice else prefix_perm(pi)
        v = np.take_along_axis(hs, sg, axis=1)  # the already sorted values indexed by Indice
        g = G[sg]
        s = g[:, 1] + g[:, 2]
        with np.errstate(all="ignore"):
            if self.kind == CHOQUET:
                I = (v[:, 0] * (f32(1) - s) + v[:, 1] * (s - g[:, 2])) + v[:, 2] * g[:, 2]
            else:
                mn = lambda a, b: np.where(a >= b, b, a)
                I = np.zeros(v.shape[0], f32)
                for t in (mn(v[:, 0], f32(1)), mn(v[:, 1], s), mn(v[:, 2], g[:, 2])):
                    I = np.where(t >= I, t, I)
        I = np.ascontiguousarray(I.astype(f32).reshape(W, H).T)
        if p["smooth"]:
            I = median3(I)
        self.integral = I
        mask = np.where(I > f32(p["threshold"]), 0, 255).astype(np.uint8)
        bgu = to_u8(bg * f32(255) + f32(0))
        fin = I[~np.isnan(I)]
        mn_ = f32(min(f32(255), fin.min())) if fin.size else f32(255)
        mx_ = f32(max(f32(0), fin.max())) if fin.size else f32(0)
        a = f32(p["alphaUpdate"])
        with np.errstate(all="ignore"):
            d = mn_ - mx_
            beta = f32(1) - (I - ((mn_ / d) * I - ((mn_ * mx_) / d)))
            beta = beta.astype(f32)[..., None]
            self.bg = (beta * bg + (f32(1) - beta) * (a * inp + (f32(1) - a) * bg)).astype(f32)
        return mask, bgu
