"""Hard masks for IndependentMultimodalBGS's area filter and the clip that injects them (not a test module; numpy only, seeded).

A detecting IMBS frame's 255-plane can be chosen freely: learn a constant background, then paint the wanted mask in a bright colour
that no earlier frame used.  `inject` builds that clip; tests/test_imbs_cpu.py asserts, through the `area_filter` hook of
imbs_numpy.run, that the plane which reaches the filter is the painted mask bit for bit, so tests/test_gpu_22_imbs_area.py compares
the device's filter (kernel_imbs.h, kernel_cc.h) with the contour-following definition of DESIGN.md §5.10 on masks of its choice.

Every generator takes (H, W, rng) with H, W >= 3 and returns a bool [H][W] with at most half of its pixels set (`sudden_change`
stays 0); the rectangles of `rect_masks` are the exception and go last in their clip."""
import functools

import numpy as np

import imbs_numpy as im

PARAMS = dict(im.DEFAULTS, numSamples=20, fps=10.0, samplingPeriod=100, minArea=2.5)  # a sample every frame, a model every 20
BACKGROUND = (40, 110, 50)
SIZES = ((33, 70), (130, 5), (5, 130), (65, 131))
RECT_SIZE = (12, 15)  # 0.6 * 180 is 108.0 in double: the contour of a 10 x 13 rectangle (9 * 12), which fills the frame's interior


def colour(t):
    return (200 - 7 * t, 220, 240 - 7 * t)


def _fit(m):
    """At most half of the pixels set: the last ones in raster order are cleared (structured masks stay below half by themselves
    at the sizes the tests use; tests/test_imbs_cpu.py asserts the properties it relies on)."""
    m = np.ascontiguousarray(m, bool)
    extra = int(m.sum()) - m.size // 2
    if extra > 0:
        flat = m.reshape(-1)
        flat[np.flatnonzero(flat)[-extra:]] = False
    return m


def _depth(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.minimum(np.minimum(yy, xx), np.minimum(H - 1 - yy, W - 1 - xx))


def _tiled(H, W, tiles, pitch):
    """The interior filled with `tiles` (cycled in raster order of the tile grid) at `pitch`, clipped at the interior's end."""
    m = np.zeros((H, W), bool)
    k = 0
    for y in range(1, H - 1, pitch):
        for x in range(1, W - 1, pitch):
            t = tiles[k % len(tiles)]
            h, w = min(t.shape[0], H - 1 - y), min(t.shape[1], W - 1 - x)
            m[y:y + h, x:x + w] = t[:h, :w]
            k += 1
    return m


def noise30(H, W, rng):
    return _fit(rng.random((H, W)) < 0.3)


def noise45(H, W, rng):
    return _fit(rng.random((H, W)) < 0.45)


def checkerboard(H, W, rng):
    """One 8-connected component; every zero with four set 4-neighbours is a hole of its own."""
    yy, xx = np.mgrid[0:H, 0:W]
    m = (yy + xx) % 2 == 0
    m[0, :] = m[-1, :] = False
    m[:, 0] = m[:, -1] = False
    return _fit(m)


def rings4(H, W, rng):
    return _fit(np.isin(_depth(H, W) % 4, (2, 3)))


def rings2(H, W, rng):
    """One-pixel rings one pixel apart: the deepest nesting the frame allows."""
    return _fit(_depth(H, W) % 2 == 1)


def comb(H, W, rng):
    m = np.zeros((H, W), bool)
    m[1, 1:W - 1] = True
    m[1:H - 1, 1:W - 1:2] = True
    return _fit(m)


def serpentine(H, W, rng):
    """One component, one pixel wide: runs on the odd rows, joined at alternating ends."""
    m = np.zeros((H, W), bool)
    m[1:H - 1:2, 1:W - 1] = True
    for y in range(2, H - 2, 2):
        m[y, W - 2 if (y // 2) % 2 else 1] = True
    return _fit(m)


def diagonals(H, W, rng):
    """8-connected lines of pitch 3, frame pixels included: no contour has an area."""
    yy, xx = np.mgrid[0:H, 0:W]
    return _fit((yy + xx) % 3 == 0)


def nested(H, W, rng):
    """A ring, a blob in its hole, a pixel hole in the blob; tiled."""
    t = np.zeros((9, 9), bool)
    t[0:7, 0:7] = True
    t[1:6, 1:6] = False
    t[2:5, 2:5] = True
    t[3, 3] = False
    return _fit(_tiled(H, W, [t], 9))


def corners(H, W, rng):
    """Blobs that touch only at a corner (one 8-connected component: two 2 x 3 blobs of area 2 make one contour of area 4, kept at
    minArea 2.5 where each alone is dropped) and holes that touch only at a corner (two 4-connected holes), on both diagonals, and
    one-pixel versions of both: the two-of-four quad with equal diagonal, in both polarities."""
    def tile(blocks, holes, side):
        t = np.zeros((7, 7), bool)
        if holes:
            t[0:side, 0:side] = True
        for y, x, h, w in blocks:
            t[y:y + h, x:x + w] = not holes
        return t
    tiles = [tile([(0, 0, 2, 3), (2, 3, 2, 3)], False, 0), tile([(1, 1, 2, 2), (3, 3, 2, 2)], True, 6), tile([(0, 3, 2, 3), (2, 0, 2, 3)], False, 0),
             tile([(1, 3, 2, 2), (3, 1, 2, 2)], True, 6), tile([(0, 0, 1, 1), (1, 1, 1, 1), (3, 4, 1, 1), (4, 3, 1, 1)], False, 0),
             tile([(1, 1, 1, 1), (2, 2, 1, 1)], True, 4), tile([(1, 2, 1, 1), (2, 1, 1, 1)], True, 4)]
    return _fit(_tiled(H, W, tiles, 7))


def frame_blobs(H, W, rng):
    """Blobs on the image frame (cleared before the contours are traced) and blobs one pixel inside it."""
    m = np.zeros((H, W), bool)
    m[0:min(4, H // 3 + 1), 0:min(5, W // 3 + 1)] = True          # on the top-left corner
    m[1:min(4, H - 1), max(W - 5, W // 2 + 1):W - 1] = True       # one pixel inside, top right
    m[H - 1, W // 3:2 * W // 3] = True                            # on the bottom frame row alone
    m[H // 2:min(H // 2 + 3, H - 1), max(W - 3, W // 2 + 1):W] = True  # on the right frame column
    m[max(H - 4, H // 2 + 1):H - 1, 1:min(4, W // 2)] = True      # one pixel inside, bottom left
    return _fit(m)


def _grid(H, W, pitch):
    m = np.zeros((H, W), bool)
    m[1:H - 1:pitch, 1:W - 1] = True
    m[1:H - 1, 1:W - 1:pitch] = True
    m[H - 2, 1:W - 1] = m[1:H - 1, W - 2] = True  # closed: the outer border is the interior's rectangle
    return m


def lattice(H, W, rng):
    """Lines every fourth row and column: one component whose outer border is too large wherever (H - 3)(W - 3) >= 0.6 H W, around
    3 x 3 holes that are kept: every pixel but the crossings survives on the border of one of its component's own holes."""
    return _fit(_grid(H, W, 4))


def sieve(H, W, rng):
    """A lattice of pitch 7 with a 4 x 4 block on every crossing that has two pixel holes touching at a corner, on alternating
    diagonals.  The outer border is too large, so a block's inner pixels live or die with those holes alone: each has area 2
    (dropped at minArea 2.5), both taken for one would have area 4."""
    m = _grid(H, W, 7)
    k = 0
    for y in range(1, H - 5, 7):
        for x in range(1, W - 5, 7):
            m[y:y + 4, x:x + 4] = True
            m[y + 1, x + 1 + k % 2] = m[y + 2, x + 2 - k % 2] = False
            k += 1
    return _fit(m)


def empty(H, W, rng):
    return np.zeros((H, W), bool)


GENERATORS = dict(noise30=noise30, noise45=noise45, checkerboard=checkerboard, rings4=rings4, rings2=rings2, comb=comb, serpentine=serpentine,
                  diagonals=diagonals, nested=nested, corners=corners, frame_blobs=frame_blobs, lattice=lattice, sieve=sieve, empty=empty)
NAMES = tuple(GENERATORS)


def masks_for(H, W, seed=0):
    """[(name, mask)] of every generator, in GENERATORS' order."""
    return [(name, g(H, W, np.random.default_rng([seed, H, W, k]))) for k, (name, g) in enumerate(GENERATORS.items())]


def rect_masks():
    """RECT_SIZE only: the filled rectangle one column narrower than the edge (area 99: kept) and the one on the edge (area 108 =
    0.6 * numPixels in double: dropped).  Both set more than half of the pixels."""
    H, W = RECT_SIZE
    narrow, full = np.zeros((H, W), bool), np.zeros((H, W), bool)
    narrow[1:H - 1, 1:W - 2] = True
    full[1:H - 1, 1:W - 1] = True
    return [("rect_below_edge", narrow), ("rect_on_edge", full)]


def clip_masks(H, W, seed=0):
    """The masks of the injected clip of one size; the rectangles last, at RECT_SIZE."""
    return masks_for(H, W, seed) + (rect_masks() if (H, W) == RECT_SIZE else [])


def inject(masks, H, W, params):
    """numSamples + 1 constant frames, then one frame per mask (bool [H][W]) painted `colour(t)`: all of them fall between the first
    build (frame numSamples - 1) and the second (frame 2 numSamples - 1, which still detects with the first model)."""
    ns, assoc = int(params["numSamples"]), int(params["associationThreshold"])
    assert 1000. / float(params["fps"]) >= float(params["samplingPeriod"]), "a sample must fall on every frame"
    assert len(masks) <= ns - 1, "the masks must end before the second build"
    cols = [colour(t) for t in range(len(masks))] + [BACKGROUND]
    for i, a in enumerate(cols):  # no bin that holds a painted colour is matched twice, so no foreground bin reaches minBinHeight (>= 2)
        for b in cols[i + 1:]:
            assert max(abs(p - q) for p, q in zip(a, b)) > assoc, (a, b)
        assert i == len(cols) - 1 or min(abs(p - q) for p, q in zip(a, BACKGROUND)) >= int(params["fgThreshold"]) and 0 <= min(a) and max(a) <= 255
    assert int(params["minBinHeight"]) >= 2
    out = np.empty((ns + 1 + len(masks), H, W, 3), np.uint8)
    out[:] = BACKGROUND
    for t, m in enumerate(masks):
        assert m.shape == (H, W) and m.dtype == bool
        out[ns + 1 + t][m] = colour(t)
    return out


def fuzz_clip(T, H, W, seed, lead):
    """The injected-mask input of the models fuzz: `lead` constant frames, then on two frames of three a seeded generator's mask
    (noise alone where a side is below 3) painted in a colour the last 18 frames did not use; the constant frames in between keep the
    background's bins the tallest at the short sample counts the fuzz draws."""
    rng = np.random.default_rng([seed, H, W])
    out = np.empty((T, H, W, 3), np.uint8)
    out[:] = BACKGROUND
    for t in range(lead, T):
        if rng.random() >= 0.65:
            continue
        g = GENERATORS[NAMES[int(rng.integers(0, len(NAMES)))]] if H >= 3 and W >= 3 else noise45
        out[t][g(H, W, rng)] = colour((t - lead) % 19)
    return out


def edge_min_area(areas2, n_pixels):
    """An area that occurs among the doubled areas `areas2` below the upper bound, a half-integer one where there is one: the median
    of the distinct ones (0.5 where no contour has an area)."""
    d = sorted({a for a in areas2 if 0 < a / 2.0 < 0.6 * n_pixels})
    d = [a for a in d if a % 2] or d
    return d[len(d) // 2] / 2.0 if d else 0.5


@functools.lru_cache(maxsize=None)
def reference(H, W, min_area=2.5, morph=0, quads=False, only=None):
    """The injected clip of one size (`only`: these generators alone, in this order) through the restatement, once: dict(names, masks,
    frames, params, first = index of the first injected frame, out = imbs_numpy.run's result, planes = what reached the area filter
    on the injected frames, stats = the filter's stats per injected frame).  Read-only."""
    named = clip_masks(H, W)
    if only is not None:
        named = [(n, dict(named)[n]) for n in only]
    names, masks = [n for n, _ in named], [m for _, m in named]
    params = dict(PARAMS, minArea=float(min_area), morphologicalFiltering=int(morph))
    frames = inject(masks, H, W, params)
    inner = im.area_filter_quads if quads else im.area_filter_follower
    planes, stats = [], []

    def hook(plane, a, _):
        planes.append(plane.copy())
        stats.append({})
        return inner(plane, a, stats[-1])
    out = im.run(params, frames, hook)
    first = params["numSamples"] + 1
    assert len(planes) == len(frames) - params["numSamples"]  # every frame after the first build reaches the filter
    for a in (frames, out[0], out[1], out[2]):
        a.setflags(write=False)
    return dict(names=names, masks=masks, frames=frames, params=params, out=out, planes=planes[1:], stats=stats[1:], first=first)


# ---- what a mask is made of (the conditions tests/test_imbs_cpu.py asserts) ------------------------------------------------------------

def structure(mask):
    """dict(holes = enclosed 4-connected zero regions, spans = the most 256-pixel spans one 8-connected component has pixels in,
    depth = the longest containment chain counted in components) of a mask after the frame is cleared."""
    H, W = mask.shape
    ones = mask.copy()
    ones[0, :] = ones[-1, :] = False
    ones[:, 0] = ones[:, -1] = False
    L1, L0 = im.label(ones, True).reshape(-1), im.label(~ones, False).reshape(-1)
    o = ones.reshape(-1)
    holes = int(np.count_nonzero((L0 == np.arange(H * W)) & ~o)) - 1
    spans = 0
    if o.any():
        pairs = np.unique(np.stack([L1[o], np.flatnonzero(o) // 256]), axis=1)
        spans = int(np.bincount(np.unique(pairs[0], return_inverse=True)[1]).max())
    depth = 0
    for g in np.flatnonzero(o & (L1 == np.arange(H * W))):
        c, d = g, 1
        while L0[c - 1] != 0:
            c, d = L1[L0[c - 1] - W], d + 1
        depth = max(depth, d)
    return dict(holes=holes, spans=spans, depth=depth)
