"""Background-rate maps for the LbpMrf mask stage, by seed: the cases of tests/golden/lbpmrf_mask_ref.npz, whose
inputs are therefore not stored.  A map is made from the sink weights it should produce: rate = 1 - (t + 0.5) / 8 truncates to t."""
import os
import zlib

import numpy as np

AREA, WEIGHT = 5, 8.0
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lbpmrf_mask_ref.npz")


def nodes(rows, cols, area=AREA):
    return rows - area + 1, (cols - area + 1) // 2


def rate_of(t):
    """f32 rates whose sink weight (short)(8 * (1 - r)) is t, for t in 0..8"""
    t = np.asarray(t, np.float32)
    return (np.float32(1) - (t + np.float32(0.5)) / np.float32(WEIGHT)).astype(np.float32)


def uniform(nh, nw, seed):
    """sink weights uniform over 0..8"""
    return rate_of(np.random.default_rng(seed).integers(0, 9, (nh, nw)))


def mostly_neutral(nh, nw, seed):
    """mostly t = 1, a few 0 and 8: units of flow travel far"""
    g = np.random.default_rng(seed)
    t = np.ones((nh, nw), np.int64)
    u = g.random((nh, nw))
    t[u < 0.12] = 0
    t[u > 0.985] = 8
    return rate_of(t)


def binary(nh, nw, seed):
    """only 0 and 8, one 8 (room for 7 units) to about seven 0 (one unit each): neither side of the cut wins outright"""
    return rate_of((np.random.default_rng(seed).random((nh, nw)) < 0.12) * 8)


def blobs(nh, nw, seed):
    """blob-like: a few soft discs of low rate on a high-rate ground, with noise, as a model's rate map looks"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:nh, 0:nw]
    r = np.full((nh, nw), 0.97, np.float64)
    for _ in range(max(3, nh * nw // 2500)):
        cy, cx, rad = g.uniform(0, nh), g.uniform(0, nw), g.uniform(2, min(max(3.0, min(nh, nw) / 5), 20.0))
        d = np.hypot(yy - cy, (xx - cx) * 2.0) / rad
        r = np.minimum(r, np.clip(d - 0.6, 0.0, 0.97))
    r = np.clip(r + g.normal(0, 0.08, (nh, nw)), 0.0, 1.0)
    return r.astype(np.float32)


def neutral(nh, nw):
    return rate_of(np.ones((nh, nw)))


def ladder(nw, mirrored):
    """two node rows: a chain in row 1 with excess (t = 0) on its first two nodes and a deficit (t = 8) on its last, pendants in row 0"""
    t = np.ones((2, nw), np.int64)
    t[1, 0] = t[1, 1] = 0
    t[1, nw - 1] = 8
    if mirrored:
        t = t[:, ::-1]
    return rate_of(np.ascontiguousarray(t))


def extremes(nh, nw):
    """all 1.0, all 0.0, a SINK ring around a SOURCE island, a single SINK node"""
    ring = np.zeros((nh, nw), np.int64)
    ring[3:nh - 3, 3:nw - 3] = 8
    ring[7:nh - 7, 7:nw - 7] = 0
    speck = np.zeros((nh, nw), np.int64)
    speck[nh // 2, nw // 2] = 8
    return np.stack([np.ones((nh, nw), np.float32), np.zeros((nh, nw), np.float32), rate_of(ring), rate_of(speck)])


MIXES = (uniform, mostly_neutral, binary)


def _small(rows, cols, count, seed):
    nh, nw = nodes(rows, cols)
    return np.stack([MIXES[k % 3](nh, nw, seed + k) for k in range(count)])


def _mix(rows, cols, per_mix, seed):
    nh, nw = nodes(rows, cols)
    # interleaved, with a trivial image among them, so that a batch mixes hard and trivial images
    maps = [MIXES[k % 3](nh, nw, seed + k) for k in range(3 * per_mix)]
    maps.insert(len(maps) // 2, neutral(nh, nw))
    return np.stack(maps)


def _large(rows, cols, seed):
    nh, nw = nodes(rows, cols)
    return np.stack([blobs(nh, nw, seed), mostly_neutral(nh, nw, seed + 1), uniform(nh, nw, seed + 2)])


def _ladder():
    return np.stack([ladder(200, False), neutral(2, 200), ladder(200, True)])


# name -> (rows, cols, maker of f32 [images][NH][NW])
CASES = {
    "one_node": (5, 6, lambda: rate_of(np.array([0, 1, 8, 3]).reshape(4, 1, 1))),
    "6x8": (6, 8, lambda: _small(6, 8, 9, 100)),
    "7x6": (7, 6, lambda: _small(7, 6, 9, 200)),
    "5x40": (5, 40, lambda: _small(5, 40, 6, 300)),
    "mix_24x44": (24, 44, lambda: _mix(24, 44, 9, 1000)),
    "mix_37x70": (37, 70, lambda: _mix(37, 70, 8, 2000)),
    "wide_70x264": (70, 264, lambda: _large(70, 264, 3000)),
    "tall_134x136": (134, 136, lambda: _large(134, 136, 4000)),
    "ladder": (6, 404, _ladder),
    "extremes": (24, 44, lambda: extremes(*nodes(24, 44))),
}


def rates(name):
    rows, cols, make = CASES[name]
    r = np.ascontiguousarray(make(), np.float32)
    assert r.shape[1:] == nodes(rows, cols), (name, r.shape)
    return rows, cols, r


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def fixture_case(z, name):
    """(masks u8 [images][rows][cols] of 0 / 255, labels u8 [images][NH][NW] with 1 = SINK, flows) of one case of the loaded fixture"""
    rows, cols, images = (int(v) for v in z[name + ".geom"])
    nh, nw = nodes(rows, cols)
    mask = np.unpackbits(z[name + ".mask"])[:images * rows * cols].reshape(images, rows, cols) * np.uint8(255)
    labels = np.unpackbits(z[name + ".labels"])[:images * nh * nw].reshape(images, nh, nw)
    return mask, labels, z[name + ".flow"]
