"""Writes tests/golden/multicue_box_ref.npz from the reference's own, unmodified SJN_MultiCueBGS (README.md here): the box stage on
hand-made landmark maps and the whole-frame step, beside tests/multicue_box_numpy.py (everything must be equal byte for byte).
usage: make_box_fixture.py /path/to/libmcboxref.so [out.npz]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import canny_numpy  # noqa: E402
import multicue_box_numpy as mb  # noqa: E402
import multicue_numpy as mc  # noqa: E402
import multicue_scenes as sc  # noqa: E402

BRANCHES = ("two_labels_one_blob", "up_plus_le", "clamp_left", "clamp_right", "clamp_upper", "clamp_bottom", "size_fails_width", "size_fails_height",
            "ghost_by_distance", "ghost_no_frame_edges", "ghost_no_fore_edges", "both_sets_empty", "valid_box", "invalid_erases_other_blob", "nn_rules_differ")


class P(C.Structure):
    _fields_ = [(k, C.c_int32 if k in mc.INT_FIELDS else C.c_float) for k in mc.FIELDS]


BOX_OUT = ("landmark", "fore0", "fore", "ghost", "update", "boxes", "dist", "count")


class BoxOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in BOX_OUT]


STATE = ("gauss", "xyz", "tbook", "tcache", "tmeans", "tcache_means", "tmeta", "tcache_meta", "tref", "tcnt", "cbook", "ccache", "cmeans", "ccache_means",
         "cmeta", "ccache_meta", "cref", "ccnt", "info")
assert STATE[:-1] == mc.STATE_PLANES


class State(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in STATE]


def box_out(rh, rw):
    a = {"landmark": np.zeros((rh, rw), np.uint8), "fore0": np.zeros((rh, rw), np.uint8), "fore": np.zeros((rh, rw), np.uint8), "ghost": np.zeros((rh, rw), np.uint8),
         "update": np.zeros((rh, rw), np.uint8), "boxes": np.zeros((mb.MAX_BOXES, 13), np.int32), "dist": np.full(mb.MAX_BOXES, -1.0), "count": np.zeros(1, np.int32)}
    return a, BoxOut(**{k: a[k].ctypes.data for k in BOX_OUT})


def cparams(full):
    return P(**{k: (int(full[k]) if k in mc.INT_FIELDS else float(full[k])) for k in mc.FIELDS})


def check_log(lib, windows):
    """the stand-in's cvCanny against tests/canny_numpy.py on every window it saw, and against the windows the restatement cut"""
    need = lib.mcb_log(None, 0)
    buf = np.zeros(max(need, 1), np.uint8)
    assert lib.mcb_log(C.c_void_p(buf.ctypes.data), need) == need
    at, calls = 0, 0
    flat = [w for gw, ea, fw, eb in windows for w in ((gw, ea), (fw, eb))]
    while at < need:
        r, c = (int(v) for v in buf[at:at + 8].view(np.int32))
        src, out = buf[at + 8:at + 8 + r * c].reshape(r, c), buf[at + 8 + r * c:at + 8 + 2 * r * c].reshape(r, c)
        assert np.array_equal(canny_numpy.canny(src, mb.CANNY_LOW, mb.CANNY_HIGH), out), "the stand-in's cvCanny differs from tests/canny_numpy.py"
        assert np.array_equal(flat[calls][0], src) and np.array_equal(flat[calls][1], out), "window %d differs from the restatement's" % calls
        at += 8 + 2 * r * c
        calls += 1
    assert calls == len(flat), (calls, len(flat))
    return calls


def count_branches(total, r, ref_dist, frame):
    """r: the restatement's result of one frame"""
    rh, rw = r["fore0"].shape
    b = r["boxes"]
    blobs, _ = mb.blobs4(r["fore0"])
    lab = r["labels"]
    for k in range(1, int(blobs.max()) + 1):
        total["two_labels_one_blob"] += len(np.unique(lab[blobs == k])) > 1
    total["up_plus_le"] += r["stats"]["up_plus_le"]
    bw, bh = rw // 80, rh // 60
    for k in range(len(b)):
        ys, xs = np.nonzero(lab == k + 1)
        total["clamp_left"] += int(xs.min() - bw < 2)
        total["clamp_right"] += int(xs.max() + bw >= rw - 2)
        total["clamp_upper"] += int(ys.min() - bh < 2)
        total["clamp_bottom"] += int(ys.max() + bh >= rh - 2)
        le, ri, up, bo, sv, v, na, nb, near = (int(x) for x in (*b[k, 0:4], *b[k, 8:13]))
        total["size_fails_width"] += not (max(rw // 32, 5) <= ri - le <= rw)
        total["size_fails_height"] += not (max(rh // 24, 5) <= bo - up <= rh)
        if sv:
            assert mb.ghost_by_count(na, nb, near) == (ref_dist[k] > 10), (k, na, nb, near, ref_dist[k])
            total["ghost_by_distance"] += na > 0 and nb > 0 and not v
            total["ghost_no_frame_edges"] += na == 0 and nb > 0 and not v
            total["ghost_no_fore_edges"] += nb == 0 and na > 0 and not v
            total["both_sets_empty"] += na == 0 and nb == 0
            total["valid_box"] += v
        if not v:
            win = r["fore0"][up:bo, le:ri] == 255
            total["invalid_erases_other_blob"] += bool((win & (lab[up:bo, le:ri] != k + 1)).any())
    nn = mb.resize_nn(frame, rh, rw)[0]
    total["nn_rules_differ"] += int((mc.reduce_frame(frame, rh, rw) != nn).any(2).sum())


def compare(name, d, ref, r):
    same = {"fore": np.array_equal(ref["fore"], r["fore"]), "ghost": np.array_equal(ref["ghost"], r["ghost"]), "update": np.array_equal(ref["update"], r["update"]),
            "count": int(ref["count"][0]) == r["count"], "boxes": np.array_equal(ref["boxes"], mb.box_rows(r["boxes"]))}
    bad = [k for k, v in same.items() if not v]
    assert not bad, (name, d, bad)
    # where the logged windows cover it, the map before any removal
    cover = np.zeros(ref["fore0"].shape, bool)
    for q in ref["boxes"][:r["count"]]:
        if q[8]:
            cover[q[2]:q[3], q[0]:q[1]] = True
    assert np.array_equal(ref["fore0"][cover], r["fore0"][cover]), (name, d, "fore0")


# name, parameters, scene, frame rows x cols, reduced rh x rw, frames, seed
STEP_CASES = [("step_12x16", mc.FAST, "scripted", 37, 53, 12, 16, 30, 21),
              ("step_30x40", mc.FAST, "scripted", 60, 85, 30, 40, 30, 22),
              ("step_half", mc.FAST, "scripted", 15, 20, 30, 40, 24, 23),
              ("step_defaults", {}, "scripted", 240, 320, 120, 160, 25, 24)]


def main():
    lib = C.CDLL(sys.argv[1])
    lib.mcb_log.restype = C.c_int64
    lib.mcb_log.argtypes = [C.c_void_p, C.c_int64]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "multicue_box_ref.npz")
    total = dict.fromkeys(BRANCHES, 0)
    z, most_labels, most_pass1, most_merges, windows_seen = {}, 0, 0, 0, 0
    posts = mb.post_inputs()
    z["post_cases"] = np.array([c[0] for c in posts])
    for name, rh, rw, rows, cols, lm, frame in posts:
        full = dict(mc.DEFAULTS, reduced_width=rw, reduced_height=rh)
        a, o = box_out(rh, rw)
        cp = cparams(full)
        rc = lib.mcb_post(C.byref(cp), rows, cols, C.c_void_p(np.ascontiguousarray(frame).ctypes.data), C.c_void_p(np.ascontiguousarray(lm).ctypes.data), C.byref(o))
        assert rc == 0, (name, rc)
        windows = []
        r = mb.boxes(lm, frame, windows)
        assert r["count"] <= mb.MAX_BOXES, name
        compare(name, 0, a, r)
        windows_seen += check_log(lib, windows)
        count_branches(total, r, a["dist"], frame)
        most_labels, most_pass1, most_merges = max(most_labels, r["count"]), max(most_pass1, r["stats"]["pass1_labels"]), max(most_merges, r["stats"]["merges"])
        n = r["count"]
        z[name + ".geom"] = np.array([rh, rw, rows, cols], np.int64)
        z[name + ".input_crc"] = np.array([mc.crc(lm), mc.crc(frame)], np.uint32)
        for k in ("fore", "ghost", "update"):
            z[name + "." + k] = np.packbits(a[k] != 0)
        z[name + ".boxes"] = a["boxes"][:n].astype(np.int16)
        z[name + ".dist"] = a["dist"][:n]
        print("%-22s %3dx%-3d <- %3dx%-3d labels %3d (pass 1 %3d, merges %3d) size-valid %3d valid %3d" % (
            name, rh, rw, rows, cols, n, r["stats"]["pass1_labels"], r["stats"]["merges"], int(a["boxes"][:n, 8].sum()), int(a["boxes"][:n, 9].sum())))
    z["step_cases"] = np.array([c[0] for c in STEP_CASES])
    for name, params, gen, rows, cols, rh, rw, T, seed in STEP_CASES:
        params = dict(params, reduced_width=rw, reduced_height=rh)
        full = dict(mc.DEFAULTS, **params)
        train = full["training_period"] + 1
        D, n = T - train, rw * rh
        frames = sc.frames_of(gen, rows, cols, T, train, seed)
        caps = (mc.T_SLOTS, mc.TCACHE_SLOTS, mc.C_SLOTS, mc.CCACHE_SLOTS)
        outs = [box_out(rh, rw) for _ in range(D)]
        images = np.zeros((T, rows, cols), np.uint8)
        st = {"gauss": np.zeros((n, 3), np.uint8), "xyz": np.zeros((n, 3), np.uint8),
              "tbook": np.zeros((n, 6, 2), np.int32), "tcache": np.zeros((n, 6, 2), np.int32),
              "tmeans": np.zeros((n, 6, caps[0]), np.float32), "tcache_means": np.zeros((n, 6, caps[1]), np.float32),
              "tmeta": np.zeros((n, 6, caps[0], 3), np.int32), "tcache_meta": np.zeros((n, 6, caps[1], 3), np.int32),
              "tref": np.zeros((n, 6), np.int16), "tcnt": np.zeros((n, 6), np.int16),
              "cbook": np.zeros((n, 2), np.int32), "ccache": np.zeros((n, 2), np.int32),
              "cmeans": np.zeros((n, caps[2], 3), np.float64), "ccache_means": np.zeros((n, caps[3], 3), np.float64),
              "cmeta": np.zeros((n, caps[2], 3), np.int32), "ccache_meta": np.zeros((n, caps[3], 3), np.int32),
              "cref": np.zeros(n, np.int16), "ccnt": np.zeros(n, np.int16), "info": np.zeros(2, np.int64)}
        cst = State(**{k: st[k].ctypes.data for k in STATE})
        couts = (BoxOut * D)(*[o for _, o in outs])
        cp = cparams(full)
        rc = lib.mcb_run(C.byref(cp), rows, cols, T, C.c_void_p(np.ascontiguousarray(frames).ctypes.data), (C.c_int * 4)(*caps), couts, C.c_void_p(images.ctypes.data), C.byref(cst))
        assert rc == 0, (name, rc)
        assert st["info"][1] == 0, "a reference book outgrew the slots"
        step = mb.Step(params)
        windows, sv, v = [], 0, 0
        for t in range(T):
            img = step.process(frames[t])
            assert np.array_equal(img, images[t]), (name, t, "image")
            if t < train:
                assert not images[t].any(), (name, t)
                continue
            d, r = t - train, step.last
            a = outs[d][0]
            assert np.array_equal(a["landmark"], step.m.landmark.reshape(rh, rw)), (name, d, "landmark")
            assert r["count"] <= mb.MAX_BOXES, name
            compare(name, d, a, r)
            # the windows of this frame, cut again for the log check
            mb.boxes(a["landmark"], frames[t], windows)
            count_branches(total, r, a["dist"], frames[t])
            most_labels, most_pass1, most_merges = max(most_labels, r["count"]), max(most_pass1, r["stats"]["pass1_labels"]), max(most_merges, r["stats"]["merges"])
            sv, v = sv + int(a["boxes"][:, 8].sum()), v + int(a["boxes"][:, 9].sum())
        windows_seen += check_log(lib, windows)
        state = step.m.state()
        bad = [k for k in mc.STATE_PLANES if state[k].tobytes() != st[k].tobytes()]
        assert not bad, (name, bad)
        assert step.m.overflow == 0 and step.box_overflow == 0 and step.m.count == st["info"][0]
        z[name + ".params"] = np.array([full[k] for k in mc.FIELDS], np.float64)
        z[name + ".scene"] = np.array([gen])
        z[name + ".geom"] = np.array([rows, cols, T, seed], np.int64)
        z[name + ".frames_crc"] = np.array([mc.crc(frames)], np.uint32)
        z[name + ".counts"] = np.array([o[0]["count"][0] for o in outs], np.int32)
        for k in ("fore", "ghost", "update"):
            z[name + "." + k] = np.packbits(np.array([o[0][k] for o in outs]) != 0)
        z[name + ".boxes"] = np.concatenate([o[0]["boxes"][:o[0]["count"][0]] for o in outs]).astype(np.int16)
        z[name + ".dist"] = np.concatenate([o[0]["dist"][:o[0]["count"][0]] for o in outs])
        if rows * cols * T <= 200000:
            z[name + ".images"] = images
        z[name + ".image_crc"] = np.array([mc.crc(im) for im in images], np.uint32)
        z[name + ".plane_crc"] = np.array([mc.crc(st[k]) for k in mc.STATE_PLANES], np.uint32)
        print("%-22s %3dx%-3d <- %3dx%-3d T=%2d labels per frame %s size-valid %d valid %d; foreground pixels of the last image %d" % (
            name, rh, rw, rows, cols, T, [int(o[0]["count"][0]) for o in outs], sv, v, int((images[-1] != 0).sum())))
    print("branches over the fixture:", total)
    print("most labels in a frame %d (pass 1: %d), most merges %d, cvCanny windows checked %d" % (most_labels, most_pass1, most_merges, windows_seen))
    missing = [k for k, v in total.items() if not v]
    assert not missing, "branches the fixture never reaches: %s" % missing
    z["branch_names"] = np.array(BRANCHES)
    z["branches"] = np.array([total[k] for k in BRANCHES], np.int64)
    np.savez_compressed(out, **z)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
