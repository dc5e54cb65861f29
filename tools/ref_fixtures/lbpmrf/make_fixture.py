"""Writes tests/golden/lbpmrf_mask_ref.npz from the reference's own, unmodified MotionDetection::GetMotionsMaskHU (README.md here):
every case of tests/lbpmrf_scenes.py, beside tests/lbpmrf_numpy.py (masks, labels and flows must be equal byte for byte).
usage: make_fixture.py /path/to/liblmref.so [out.npz] [--time-1080p]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lbpmrf_numpy as ln  # noqa: E402
import lbpmrf_scenes as sc  # noqa: E402

BRANCHES = ("node_255", "node_0", "between_255", "between_0", "left_bound_fails", "right_bound_fails", "up_bound_fails", "down_bound_fails", "stranded")


def reference(lib, rate, rows, cols, area=sc.AREA, weight=sc.WEIGHT):
    nh, nw = rate.shape
    mask, labels = np.zeros((rows, cols), np.uint8), np.zeros((nh, nw), np.uint8)
    flow, secs = C.c_int32(0), C.c_double(0)
    rate = np.ascontiguousarray(rate, np.float32)
    rc = lib.lm_run(rows, cols, area, C.c_float(weight), C.c_void_p(rate.ctypes.data), C.c_void_p(mask.ctypes.data), C.c_void_p(labels.ctypes.data), C.byref(flow), C.byref(secs))
    assert rc == 0, rc
    return mask, labels, int(flow.value), secs.value


def time_1080p(lib):
    """the reference's own maxflow() on the maps of the bench leg (tools/bench_configs.py --only lbpmrf_mask), this CPU, one run each"""
    rows, cols = 1080, 1920
    nh, nw = sc.nodes(rows, cols)
    for name, rate in (("blobs", sc.blobs(nh, nw, 1)), ("noise", sc.uniform(nh, nw, 2)), ("neutral", sc.neutral(nh, nw))):
        t0 = time.perf_counter()
        mask, labels, flow, secs = reference(lib, rate, rows, cols)
        print("1080p %-8s %d x %d nodes: maxflow() %.1f ms, the whole driver call around GetMotionsMaskHU %.1f ms, flow %d, SINK nodes %d" % (
            name, nh, nw, secs * 1e3, (time.perf_counter() - t0) * 1e3, flow, int(labels.sum())))


def main():
    lib = C.CDLL(sys.argv[1])
    args = [a for a in sys.argv[2:] if not a.startswith("--")]
    out = args[0] if args else os.path.join(ROOT, "tests", "golden", "lbpmrf_mask_ref.npz")
    total = dict.fromkeys(BRANCHES, 0)
    z = {"cases": np.array(list(sc.CASES))}
    for name in sc.CASES:
        rows, cols, rates = sc.rates(name)
        masks, labels, flows = [], [], []
        for i, rate in enumerate(rates):
            m, lab, f, _ = reference(lib, rate, rows, cols)
            rm, rl, rf = ln.lbpmrf_mask(rate, rows, cols, stats=total)
            assert np.array_equal(m, rm), (name, i, "mask")
            assert np.array_equal(lab, rl), (name, i, "labels")
            assert f == rf, (name, i, "flow", f, rf)
            t = ln.sink_weights(rate)
            assert ln.duality(t, lab) == f, (name, i, "duality")
            assert set(np.unique(m)) <= {0, 255}
            masks.append(m), labels.append(lab), flows.append(f)
        masks, labels = np.array(masks), np.array(labels)
        z[name + ".geom"] = np.array([rows, cols, len(rates)], np.int64)
        z[name + ".rate_crc"] = np.array([sc.crc(rates)], np.uint32)
        z[name + ".mask"] = np.packbits(masks != 0)
        z[name + ".labels"] = np.packbits(labels != 0)
        z[name + ".flow"] = np.array(flows, np.int32)
        print("%-14s %3d x %-3d %2d maps: SINK nodes %s flows %s foreground pixels %s" % (
            name, rows, cols, len(rates), [int(v.sum()) for v in labels][:6], flows[:6], [int((v != 0).sum()) for v in masks][:6]))
    # the hand-readable expectations of the issue's cases
    rows, cols, rates = sc.rates("extremes")
    ex_m = np.unpackbits(z["extremes.mask"])[:4 * rows * cols].reshape(4, rows, cols)
    ex_l = np.unpackbits(z["extremes.labels"])[:rates.size].reshape(rates.shape)
    assert not ex_l[0].any() and not ex_m[0].any(), "all rates 1.0: everything SOURCE, empty mask"
    assert ex_l[1].all(), "all rates 0.0: everything SINK"
    nh, nw = rates.shape[1:]
    assert not ex_l[2, nh // 2, nw // 2] and ex_m[2, nh // 2 + 3, 2 * (nw // 2) + 2], "the SOURCE island inside the SINK ring is a hole that step 5 fills"
    assert ex_l[3].sum() == 1 and not ex_m[3].any(), "a single SINK node is a speck that step 6 erases"
    rows, cols, rates = sc.rates("ladder")
    la = np.unpackbits(z["ladder.labels"])[:rates.size].reshape(rates.shape)
    print("ladder: SOURCE nodes of the three maps", [np.argwhere(v == 0).tolist() if (v == 0).sum() < 8 else int((v == 0).sum()) for v in la])
    print("branches over the fixture:", total)
    missing = [k for k, v in total.items() if not v]
    assert not missing, "branches the fixture never reaches: %s" % missing
    z["branch_names"] = np.array(BRANCHES)
    z["branches"] = np.array([total[k] for k in BRANCHES], np.int64)
    np.savez_compressed(out, **z)
    print(out, os.path.getsize(out), "bytes")
    if "--time-1080p" in sys.argv:
        time_1080p(lib)


if __name__ == "__main__":
    main()
