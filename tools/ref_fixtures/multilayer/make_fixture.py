"""Writes tests/golden/multilayer_ref.npz and tests/golden/multilayer_fuzz_ref.npz from the reference's own model code (README.md here).
The second file pins the restatement where the models fuzz takes it: every stream of every accepted case of the fixed MultiLayerBGS
slices of tests/model_refs.py, run straight through (no reset) with the case's parameters, as CRCs.
usage: make_fixture.py /path/to/libmlref.so [out.npz [fuzz_out.npz]]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)  # tests/model_refs.py names the class ids of tracking_amd.capi
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multilayer_numpy as ml  # noqa: E402
import multilayer_scenes as sc  # noqa: E402

FULL_MODES_BELOW = 400  # pixels: larger cases store the CRC of the modes plane instead of its 360 bytes per pixel


class P(C.Structure):
    _fields_ = [(k, C.c_int32 if k in ml.INT_FIELDS else C.c_float) for k in ml.FIELDS]


SIZES = [(3, 3), (5, 7), (9, 4), (130, 5), (5, 130), (65, 131)]  # rows x cols
CASES = [("defaults", {}, "static_block", 37, 53, 24, 11),
         ("fast", ml.FAST, "scripted", 37, 53, 40, 12),
         ("K1", dict(ml.FAST, max_mode_num=1), "scripted", 12, 16, 20, 13),
         ("K3", dict(ml.FAST, max_mode_num=3), "scripted", 12, 16, 20, 14),
         ("detect_after", dict(ml.FAST, detect_after=8), "scripted", 12, 16, 18, 15),
         ("detect_after_nolearn", dict(ml.FAST, detect_after=8, disable_learning=1), "scripted", 12, 16, 18, 15),
         ("status_detect", dict(disable_detect_mode=0, status=1), "static_block", 12, 16, 12, 16),
         ("no_texture", dict(ml.FAST, texture_weight=0.0), "scripted", 12, 16, 20, 17),
         ("no_smooth", dict(ml.FAST, pattern_neig_half_size=-1), "scripted", 12, 16, 16, 18),
         ("h0", dict(ml.FAST, pattern_neig_half_size=0), "scripted", 12, 16, 16, 19),
         ("dark", dict(ml.FAST), "dark", 16, 20, 16, 20)]
CASES += [("fast_%dx%d" % rc, ml.FAST, "scripted", rc[0], rc[1], 12, 30 + i) for i, rc in enumerate(SIZES)]


def run_reference(lib, params, frames):
    T, rows, cols = frames.shape[:3]
    n = rows * cols
    p = P(**{k: (int(v) if k in ml.INT_FIELDS else float(v)) for k, v in dict(ml.DEFAULTS, **params).items()})
    masks, bgs = np.zeros((T, rows, cols), np.uint8), np.zeros((T, rows, cols, 3), np.uint8)
    order, modes, dist = np.zeros((n, 7), np.uint8), np.zeros((n, 5, 18), np.float32), np.zeros(n, np.float32)
    consts, counts = np.zeros(2, np.uint32), np.zeros(2, np.int64)
    fr = np.ascontiguousarray(frames)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.ml_run(C.byref(p), rows, cols, T, ptr(fr), ptr(masks), ptr(bgs), ptr(order), ptr(modes), ptr(dist), ptr(consts), ptr(counts))
    assert rc == 0
    return masks, bgs, order, modes, dist, consts, counts


def fuzz_runs():
    """(case, stream, frames) of every accepted case of the fixed slices; tests/test_multilayer_cpu.py draws the same."""
    import model_refs as mr
    ad = mr.BY_CLASS[ml.CLASS_NAME]
    for _, classes, big, first, count in mr.SLICES:
        if classes != (ml.CLASS_NAME,):
            continue
        for case in mr.slice_cases(first, count, classes, big):
            if ad.refusal(ml.CLASS_NAME, case["params"]) is None:
                for s, frames in enumerate(mr.build_inputs(case)):
                    yield case, s, frames


def write_fuzz_fixture(lib, out):
    """Per run: (seed, stream), the CRC-32 of the input, the masks, the backgrounds, `order`, `modes` and `dist` after the last frame,
    and the expf call / libm-differs counts.  The counts are recorded, not conditioned on: the model gets the correctly rounded value
    either way."""
    runs, crcs, expf, differ = [], [], [], 0
    for case, s, frames in fuzz_runs():
        masks, bgs, order, modes, dist, consts, counts = run_reference(lib, case["params"], frames)
        ref = [ml.crc(frames), ml.crc(masks), ml.crc(bgs), ml.crc(order), ml.crc(modes), ml.crc(dist)]
        m, rm, rb = ml.run(case["params"], frames, int(consts[0]))
        mine = [ref[0], ml.crc(rm), ml.crc(rb)] + [ml.crc(a) for a in m.state()]
        if mine != ref:
            differ += 1
            print("seed %d stream %d %dx%d T=%d: restatement differs (input masks bg order modes dist) %s %s" % (case["seed"], s, case["H"], case["W"], case["T"],
                  [a == b for a, b in zip(mine, ref)], case["params"]))
        runs.append((case["seed"], s)), crcs.append(ref), expf.append([int(counts[0]), int(counts[1])])
    np.savez_compressed(out, runs=np.array(runs, np.int64), crcs=np.array(crcs, np.uint32), expf=np.array(expf, np.int64))
    print("%s: %d runs, %d where the restatement differs, %d with an expf call where libm differs, %d bytes" % (out, len(runs), differ, sum(e[1] > 0 for e in expf), os.path.getsize(out)))


def main():
    lib = C.CDLL(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "multilayer_ref.npz")
    z, total = {"cases": np.array([c[0] for c in CASES])}, dict.fromkeys(ml.COUNTERS, 0)
    for name, params, gen, rows, cols, T, seed in CASES:
        for attempt in range(20):  # only cases where libm's expf is the correctly rounded value in every call are kept
            frames = sc.frames_of(gen, rows, cols, T, seed)
            masks, bgs, order, modes, dist, consts, counts = run_reference(lib, params, frames)
            if not counts[1]:
                break
            print("%s: seed %d: libm's expf differs from the correctly rounded value in %d of %d calls: next seed" % (name, seed, counts[1], counts[0]))
            seed += 100
        assert not counts[1]
        full = dict(ml.DEFAULTS, **params)
        z[name + ".params"] = np.array([full[k] for k in ml.FIELDS], np.float64)
        z[name + ".scene"] = np.array([gen])
        z[name + ".geom"] = np.array([rows, cols, T, seed], np.int64)
        z[name + ".frames_crc"] = np.array([ml.crc(frames)], np.uint32)
        z[name + ".masks"] = masks
        z[name + ".bg_crc"] = np.array([ml.crc(b) for b in bgs], np.uint32)
        z[name + ".order"] = order
        z[name + ".modes_crc"] = np.array([ml.crc(modes)], np.uint32)
        if rows * cols < FULL_MODES_BELOW:
            z[name + ".modes"] = modes
        z[name + ".dist"] = dist
        z[name + ".consts"] = consts
        z[name + ".expf"] = counts
        m, rm, rb = ml.run(params, frames, int(consts[0]))
        o2, m2, d2 = m.state()
        same = (np.array_equal(rm, masks), np.array_equal(rb, bgs), np.array_equal(o2, order), m2.tobytes() == modes.tobytes(), d2.tobytes() == dist.tobytes())
        for k in total:
            total[k] += m.counts[k]
        print("%-22s %3dx%-3d T=%2d fg %.3f expf %d/%d restatement masks/bg/order/modes/dist %s %s" % (name, rows, cols, T, (masks == 255).mean(), counts[1], counts[0], same, {k: v for k, v in m.counts.items() if v}))
    print("counters over the fixture:", total)
    np.savez_compressed(out, **z)
    print(out, os.path.getsize(out), "bytes")
    write_fuzz_fixture(lib, sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "tests", "golden", "multilayer_fuzz_ref.npz"))


if __name__ == "__main__":
    main()
