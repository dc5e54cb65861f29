"""The five package_bgs/dp models pinned by the reference's own code (not a test module): the cases, their seeded input clips and
the reader of tests/golden/dp_ref_{ziv,grim,wren,mean,median}.npz.  tests/golden/make_dp_ref.py writes those files from
oracle/_ref/ref_dp_cli (the reference's model files compiled unmodified, oracle/Makefile); tests/test_dp_cpu.py compares the CPU
oracle with them and tests/test_gpu_14_dp_ref.py the HIP kernels.

A case's `params` hold the WRAPPER's values in the wrapper's types (threshold: int for mean and median, double otherwise), so a
threshold of 130 or -1 is what an edited config/DP*.xml would hold; the truncations that follow are the reference's own."""
import io
import json
import os
import zipfile
import zlib

import numpy as np

from tracking_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

CLASSES = {  # key -> (host class, algorithm, state planes as (name, dtype))
    "ziv": ("DPZivkovicAGMMBGS", capi.DP_ZIVKOVIC_AGMM, ("modes", "nmodes")),
    "grim": ("DPGrimsonGMMBGS", capi.DP_GRIMSON_GMM, ("modes", "nmodes")),
    "wren": ("DPWrenGABGS", capi.DP_WREN_GA, ("gauss",)),
    "mean": ("DPMeanBGS", capi.DP_MEAN, ("mean",)),
    "median": ("DPAdaptiveMedianBGS", capi.DP_ADAPTIVE_MEDIAN, ("median",)),
}
FIELDS = {"ziv": 5, "grim": 6}
f32 = lambda v: float(np.float32(v))  # noqa: E731  the wrappers' float literals, widened to their double members
DEFAULTS = {  # the constructors of DP*BGS.cpp:19
    "ziv": dict(threshold=25.0, alpha=f32(0.001), gaussians=3),
    "grim": dict(threshold=9.0, alpha=0.01, gaussians=3),
    "wren": dict(threshold=12.25, alpha=f32(0.005), learning_frames=30),
    "mean": dict(threshold=2700, alpha=f32(1e-6), learning_frames=30),
    "median": dict(threshold=40, sampling_rate=7, learning_frames=30),
}
PLANE_PIXELS = 1000  # whole-model planes are stored for cases of at most about this many pixels

RAGGED = "random:12:37:53:5"  # 1 961 pixels: no multiple of 4 or of the 256-pixel state tile; cases take 10-frame windows of it
TILE = "random:12:16:64:6"    # 1 024 pixels: exactly four tiles, npix % 4 == 0
SMALL = "random:12:9:13:7"    # 117 pixels: the parameter cases
MODES = "modes:40:8:14:8"
TIES = "ties:30:10:16:9"


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def random_clip(T, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (T, H, W, 3), dtype=np.uint8)


def modes_clip(T, H, W, seed):
    """Every pixel dwells on one of six colours of its own for a random stretch, with small noise (lb_numpy.modes_clip with a larger
    palette, so that K = 5 fills up too): the GMMs fill their K modes, replace the last one and re-sort."""
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, (6, H, W, 3)).astype(np.int16)
    pal[1] = np.clip(pal[0] + rng.integers(-25, 26, (H, W, 3)), 0, 255)  # a near neighbour: matched by the same mode or not
    out = np.empty((T, H, W, 3), np.uint8)
    cur = np.zeros((H, W), np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    for t in range(T):
        cur = np.where(rng.random((H, W)) < 0.3, rng.integers(0, 6, (H, W)), cur)
        out[t] = np.clip(pal[cur, yy, xx] + rng.integers(-3, 4, (H, W, 3)), 0, 255)
    return out


def ties_clip(T, H, W, seed):
    """Bytes 0 / 128 / 255 only; a pixel alternates between two or three such colours in runs of equal length, so modes with equal
    weights, equal variances (on the clamp) and equal Grimson sort keys are common, and distances are equal or zero."""
    rng = np.random.default_rng(seed)
    lv = np.array([0, 128, 255], np.uint8)
    pal = lv[rng.integers(0, 3, (3, H, W, 3))]
    period = rng.integers(1, 4, (H, W))
    ncol = rng.integers(2, 4, (H, W))
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty((T, H, W, 3), np.uint8)
    for t in range(T):
        out[t] = pal[(t // period) % ncol, yy, xx]
    return out


def clip(spec):
    if spec == "long72":  # the clip of test_dp_models_long_clip_with_scene_changes: frames_96x80, its +60 copy, then its reverse
        g = np.load(os.path.join(GOLDEN, "frames_96x80.npz"))["frames"]
        return np.concatenate([g, np.clip(g.astype(np.int32) + 60, 0, 255).astype(np.uint8), g[::-1]])
    kind, T, H, W, seed = spec.split(":")
    return {"random": random_clip, "modes": modes_clip, "ties": ties_clip}[kind](int(T), int(H), int(W), int(seed))


def cases(cls):
    """Ordered {case: params}.  params = the wrapper's values + `input` (clip spec) + optional `window` [t0, t1)."""
    d = DEFAULTS[cls]
    c = {}

    def add(name, inp, window=None, **kw):
        p = dict(d, input=inp, **kw)
        if window:
            p["window"] = list(window)
        c[name] = p

    add("default", "long72")
    add("ragged", RAGGED, (0, 10))
    add("ragged_o1", RAGGED, (1, 11))  # the same clip entered one and two frames later: the streams of the batch test
    add("ragged_o2", RAGGED, (2, 12))
    add("tile", TILE)
    add("tiny5x7", "random:12:5:7:3")
    add("tiny1x1", "random:12:1:1:4")
    # GMMs: an alpha below float's epsilon - 1 - alpha rounds to 1, old weights stay 1 and every later mode gets weight alpha, so
    # equal weights, equal variances and equal Grimson sort keys are certain (no such tie was met at alpha 0.5, 0.25, 0.01, ...)
    add("ties", TIES, **({"alpha": f32(1e-8)} if cls in FIELDS else {}))
    if cls in FIELDS:
        add("modes", MODES)
        for K in (1, 2, 4, 5):
            add("modes_k%d" % K, MODES, gaussians=K)
        add("alpha03", MODES, alpha=f32(0.3))
        add("alpha06_k4", MODES, alpha=f32(0.6), gaussians=4)
        add("modes_ties", MODES, alpha=f32(1e-8))  # `modes` itself meets no equal keys at the default alpha: this twin does
        add("thr2", SMALL, threshold=2.0)
    else:
        add("modes", MODES)
        add("learn0", RAGGED, (0, 10), learning_frames=0)  # must equal `ragged`: the update mask is always background
    if cls == "wren":
        add("thr1", SMALL, threshold=1.0)
        add("thr40", SMALL, threshold=40.0)
        add("alpha05", SMALL, alpha=0.5)
    if cls == "mean":
        add("alpha05", SMALL, alpha=0.5)
        add("alpha09", SMALL, alpha=f32(0.9))
        for t in (0, -1, 5000):
            add("t%d" % t, SMALL, threshold=t)
    if cls == "median":
        for t in (0, 44, 100, 127, 128, 130, 200, 255, 256, 300, -1):
            add("t%d" % t, SMALL, threshold=t, sampling_rate=2)
        for r in (1, 2, 7):
            add("rate%d" % r, SMALL, sampling_rate=r)
        for t in (130, 300):  # the wrap on both kernel forms: npix % 4 == 0 and an odd pixel count
            add("tile_t%d" % t, TILE, threshold=t)
            add("ragged_t%d" % t, RAGGED, (0, 10), threshold=t)
    return c


def frames_of(p):
    f = clip(p["input"])
    if "window" in p:
        f = f[p["window"][0]:p["window"][1]]
    return np.ascontiguousarray(f)


def ref_kwargs(cls, p):
    """The key=value arguments of oracle/ref_dp_cli for a case."""
    kw = dict(threshold=p["threshold"])
    if "alpha" in p:
        kw["alpha"] = p["alpha"]
    if "gaussians" in p:
        kw["gaussians"] = p["gaussians"]
    if "sampling_rate" in p:
        kw["rate"] = p["sampling_rate"]
    if "learning_frames" in p:
        kw["learn"] = p["learning_frames"]
    return kw


def engine_params(cls, p):
    """bgs_params of a case, as the host classes fill them from the wrapper's members (bgs_classes.inc: `(float)threshold`)."""
    q = capi.default_params(CLASSES[cls][1])
    q.dp_threshold = float(p["threshold"])
    if "alpha" in p:
        q.dp_alpha = p["alpha"]
    if "gaussians" in p:
        q.dp_gaussians = p["gaussians"]
    if "sampling_rate" in p:
        q.dp_sampling_rate = p["sampling_rate"]
    if "learning_frames" in p:
        q.learning_frames = p["learning_frames"]
    return q


def plane_shape(cls, plane, p, n):
    if plane == "modes":
        return (p["gaussians"] * FIELDS[cls], n), np.float32
    return {"nmodes": ((n,), np.uint8), "gauss": ((4, n), np.float32), "mean": ((3, n), np.float32), "median": ((n, 3), np.uint8)}[plane]


# ---- the fixture files: a zip of .npy members like np.savez, written with fixed timestamps so that a rerun gives the same bytes

def save(path, arrays):
    with zipfile.ZipFile(path, "w") as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


_loaded = {}


def load(cls):
    """{case: record}; a record holds params (dict), frames (the input, CRC-checked), masks [T][H][W] and the stored planes."""
    if cls not in _loaded:
        z = np.load(os.path.join(GOLDEN, "dp_ref_%s.npz" % cls))
        out = {}
        for case in json.loads(str(z["cases"])):
            r = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(case + "/")}
            p = json.loads(str(r["params"]))
            frames = frames_of(p)
            assert crc(frames) == int(r["input_crc32"]), "%s/%s: the input clip differs from the one the fixture was made from" % (cls, case)
            T, H, W = (int(v) for v in r["shape"])
            assert frames.shape == (T, H, W, 3)
            masks = np.unpackbits(r["masks"], axis=-1)[..., :W].reshape(T, H, W) * np.uint8(255)
            planes = {}
            for name in CLASSES[cls][2]:
                if name in r:
                    shape, dt = plane_shape(cls, name, p, H * W)
                    planes[name] = r[name].view(dt).reshape(shape)  # floats are stored as their bits (uint32)
            out[case] = dict(params=p, frames=frames, masks=masks, planes=planes)
            for a in (frames, masks, *planes.values()):
                a.setflags(write=False)
        _loaded[cls] = (out, json.loads(str(z["environment"])))
    return _loaded[cls][0]


def environment(cls):
    load(cls)
    return _loaded[cls][1]


def oracle_run(cls, p, frames, want_planes=()):
    """The CPU oracle on a case: masks [T][H][W] and the requested planes after the last frame."""
    from oracle import pyoracle
    o = pyoracle.Oracle(CLASSES[cls][1], params=engine_params(cls, p))
    masks = np.array([o.process(f, want_bg=False)[0] for f in frames])
    n = frames.shape[1] * frames.shape[2]
    planes = {name: o.get_state(name, *plane_shape(cls, name, p, n)) for name in want_planes}
    o.close()
    return masks, planes


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
