"""Writes tests/golden/multicue_ref.npz from the reference's own, unmodified SJN_MultiCueBGS (README.md here).
usage: make_fixture.py /path/to/libmcref.so [out.npz]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multicue_numpy as mc  # noqa: E402
import multicue_scenes as sc  # noqa: E402

FULL_PLANES_BELOW = 100  # reduced pixels: larger cases store the CRC of every state plane only

# name, parameters, scene, frame rows x cols, reduced rh x rw, frames, seed
CASES = [("fast_5x5", mc.FAST, "scripted", 37, 53, 5, 5, 40, 11),
         ("fast_6x9", mc.FAST, "scripted", 37, 53, 6, 9, 40, 12),
         ("fast_12x16", mc.FAST, "scripted", 37, 53, 12, 16, 40, 13),
         ("fast_24x20", mc.FAST, "scripted", 37, 53, 24, 20, 40, 14),
         ("small_frame", mc.FAST, "scripted", 7, 9, 12, 16, 40, 15),
         ("no_absorption", dict(mc.FAST, absorption_enable=0), "scripted", 37, 53, 12, 16, 40, 16),
         ("drift", mc.FAST, "drift", 12, 16, 12, 16, 70, 17),
         ("defaults", {}, "scripted", 240, 320, 120, 160, 25, 18)]


class P(C.Structure):
    _fields_ = [(k, C.c_int32 if k in mc.INT_FIELDS else C.c_float) for k in mc.FIELDS]


IO_FIELDS = ("frames", "ghost", "boxes", "landmark", "conf", "update", "gauss", "xyz", "tbook", "tcache", "tmeans", "tcache_means", "tmeta", "tcache_meta", "tref", "tcnt",
             "cbook", "ccache", "cmeans", "ccache_means", "cmeta", "ccache_meta", "cref", "ccnt", "info")


class IO(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in IO_FIELDS]


def run_reference(lib, params, frames, ghost, boxes):
    p = dict(mc.DEFAULTS, **params)
    rw, rh, n = p["reduced_width"], p["reduced_height"], p["reduced_width"] * p["reduced_height"]
    T, rows, cols = frames.shape[:3]
    D = T - (p["training_period"] + 1)
    caps = (mc.T_SLOTS, mc.TCACHE_SLOTS, mc.C_SLOTS, mc.CCACHE_SLOTS)
    a = {"frames": np.ascontiguousarray(frames), "ghost": np.ascontiguousarray(ghost), "boxes": np.ascontiguousarray(boxes),
         "landmark": np.zeros((D, rh, rw), np.uint8), "conf": np.zeros((D, rh, rw), np.float32), "update": np.zeros((D, rh, rw), np.uint8),
         "gauss": np.zeros((n, 3), np.uint8), "xyz": np.zeros((n, 3), np.uint8),
         "tbook": np.zeros((n, 6, 2), np.int32), "tcache": np.zeros((n, 6, 2), np.int32),
         "tmeans": np.zeros((n, 6, caps[0]), np.float32), "tcache_means": np.zeros((n, 6, caps[1]), np.float32),
         "tmeta": np.zeros((n, 6, caps[0], 3), np.int32), "tcache_meta": np.zeros((n, 6, caps[1], 3), np.int32),
         "tref": np.zeros((n, 6), np.int16), "tcnt": np.zeros((n, 6), np.int16),
         "cbook": np.zeros((n, 2), np.int32), "ccache": np.zeros((n, 2), np.int32),
         "cmeans": np.zeros((n, caps[2], 3), np.float64), "ccache_means": np.zeros((n, caps[3], 3), np.float64),
         "cmeta": np.zeros((n, caps[2], 3), np.int32), "ccache_meta": np.zeros((n, caps[3], 3), np.int32),
         "cref": np.zeros(n, np.int16), "ccnt": np.zeros(n, np.int16), "info": np.zeros(8, np.int64)}
    io = IO(**{k: a[k].ctypes.data for k in IO_FIELDS})
    cp = P(**{k: (int(p[k]) if k in mc.INT_FIELDS else float(p[k])) for k in mc.FIELDS})
    rc = lib.mc_run(C.byref(cp), rows, cols, T, boxes.shape[1], (C.c_int * 4)(*caps), C.byref(io))
    assert rc == 0, rc
    return a


def main():
    lib = C.CDLL(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "multicue_ref.npz")
    z, total, maxima = {"cases": np.array([c[0] for c in CASES])}, dict.fromkeys(mc.COUNTERS, 0), np.zeros(4, np.int64)
    for name, params, gen, rows, cols, rh, rw, T, seed in CASES:
        params = dict(params, reduced_width=rw, reduced_height=rh)
        full = dict(mc.DEFAULTS, **params)
        train = full["training_period"] + 1
        frames = sc.frames_of(gen, rows, cols, T, train, seed)
        ghost, boxes = sc.maps_of(gen, rh, rw, T - train)
        ref = run_reference(lib, params, frames, ghost, boxes)
        info = ref["info"]
        assert info[5] == 0, "a stored threshold is not mean -/+ (float)range"
        assert info[6] == 0, "a reference book outgrew the slots"
        assert info[0] == full["training_period"] + 2
        for d in range(T - train):
            assert np.array_equal(ref["update"][d], sc.update_map_of(boxes[d], rh, rw)), d
        m, lms, confs = mc.run(params, frames, ghost, ref["update"])
        st = m.state()
        same = {"landmark": np.array_equal(lms, ref["landmark"]), "conf": confs.tobytes() == ref["conf"].tobytes()}
        for k in mc.STATE_PLANES:
            same[k] = st[k].tobytes() == ref[k].tobytes()
        bad = [k for k, v in same.items() if not v]
        assert not bad, (name, bad)
        assert m.overflow == 0 and m.count == info[0]
        maxima = np.maximum(maxima, info[1:5])
        for k in total:
            total[k] += m.counts[k]
        z[name + ".params"] = np.array([full[k] for k in mc.FIELDS], np.float64)
        z[name + ".scene"] = np.array([gen])
        z[name + ".geom"] = np.array([rows, cols, T, seed], np.int64)
        z[name + ".frames_crc"] = np.array([mc.crc(frames)], np.uint32)
        z[name + ".landmark"] = ref["landmark"]
        z[name + ".conf"] = ref["conf"]
        z[name + ".update"] = ref["update"]
        z[name + ".count"] = info[:1].copy()
        z[name + ".maxima"] = info[1:5].copy()
        z[name + ".plane_crc"] = np.array([mc.crc(ref[k]) for k in mc.STATE_PLANES], np.uint32)
        if rw * rh < FULL_PLANES_BELOW:
            for k in mc.STATE_PLANES:
                z[name + "." + k] = ref[k]
        print("%-14s %3dx%-3d -> %3dx%-3d T=%2d landmark 255/125 %.3f/%.3f largest books %s restatement equal; %s" % (
            name, rows, cols, rh, rw, T, (ref["landmark"] == 255).mean(), (ref["landmark"] == 125).mean(), list(info[1:5]), {k: v for k, v in m.counts.items() if v}))
    print("counters over the fixture:", total)
    print("largest m_iNumEntries (texture, texture cache, colour, colour cache):", list(maxima))
    missing = [k for k, v in total.items() if not v]
    assert not missing, "branches the fixture never reaches: %s" % missing
    assert (2 * maxima <= np.array([mc.T_SLOTS, mc.TCACHE_SLOTS, mc.C_SLOTS, mc.CCACHE_SLOTS])).all(), "the slots are less than twice the measured maxima"
    z["counter_names"] = np.array(mc.COUNTERS)
    z["counters"] = np.array([total[k] for k in mc.COUNTERS], np.int64)
    z["maxima"] = maxima
    np.savez_compressed(out, **z)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
