"""IndependentMultimodalBGS (USTC_BGS type 33's class) without a GPU: the numpy restatement against the fixture made from the
reference's own db/imbs.cpp, the two forms of the area filter against each other, the conditions that make the fixture a fair
yardstick, the C ABI (ids, bgs_imbs_params, the refusals) and the host layer (class list, XML, the type table, the FrameProcessor
flag, the reference-side adapters)."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import imbs_masks as mk
import imbs_numpy as im
from tracking_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "tracking_amd", "host")
FIELDS = [f for f, _ in capi.BgsImbsParams._fields_]
HOLES = ("holes_a0", "holes_a2", "holes_a30", "holes_big")


@functools.lru_cache(maxsize=None)
def restated(case, quads=False):
    r = im.load()[case]
    return im.run(r["params"], r["frames"], im.area_filter_quads if quads else im.area_filter_follower)


# ---- the restatement and the fixture -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(im.cases()))
def test_restatement_reproduces_the_reference_fixture(case):
    r = im.load()[case]
    masks, bgs, ctl, mdl = restated(case)
    assert np.array_equal(masks, r["masks"])
    assert [im.crc(b) for b in bgs] == [int(c) for c in r["bg_crc"]]
    assert ctl.tobytes() == r["control"].tobytes()
    n = masks.shape[1] * masks.shape[2]
    assert ("bins" in r) == (n <= im.PLANE_PIXELS)
    if "bins" in r:
        for pl, v in mdl.planes().items():
            assert v.tobytes() == r[pl].tobytes(), pl


@pytest.mark.parametrize("case", HOLES + ("basic", "sudden", "morph"))
def test_quad_form_gives_the_same_masks_on_the_fixture(case):
    a, b = restated(case), restated(case, True)
    assert np.array_equal(a[0], b[0]) and a[2].tobytes() == b[2].tobytes()


def test_follower_form_equals_quad_form_on_random_masks():
    """1 200 seeded masks up to 14 x 14, pixels on the image frame set, every fifth one two nested rings around noise, each at four
    values of minArea: the contract (border follower, polygon area, polygon fill) and the device's form keep the same pixels."""
    rng = np.random.default_rng(5)
    contours = 0
    for it in range(1200):
        H, W = int(rng.integers(3, 15)), int(rng.integers(3, 15))
        m = rng.random((H, W)) < rng.choice([0.45, 0.6, 0.75, 0.9])
        if it % 5 == 0 and H > 8 and W > 8:
            m[:] = False
            m[1:-1, 1:-1] = True
            m[2:-2, 2:-2] = False
            m[3:-3, 3:-3] = True
            m[4:-4, 4:-4] = rng.random((H - 8, W - 8)) < 0.5
            m[0, ::2] = True  # frame pixels never survive
        contours += len(im.contours(m))
        for min_area in (0.0, 0.5, 2.5, 6.0):
            a, b = im.area_filter_follower(m, min_area), im.area_filter_quads(m, min_area)
            assert np.array_equal(a, b), (it, min_area, m.astype(int))
            assert not a[0].any() and not a[-1].any() and not a[:, 0].any() and not a[:, -1].any()
    assert contours >= 2 * 1200  # the masks are not trivial: two borders a mask on average at the least


def test_every_branch_of_the_survival_rule_is_taken_in_the_holes_cases():
    stats = {}
    for case in HOLES:
        r = im.load()[case]
        m = im.Model(r["params"], *r["frames"].shape[1:3], area_filter=im.area_filter_quads)
        for f in r["frames"]:
            m.apply(f)
        for k, v in m.stats.items():
            stats[k] = stats.get(k, 0) + v
    assert stats.get("chain", 0) > 0 and stats.get("own_hole", 0) > 0 and stats.get("dropped", 0) > 0, stats
    follower = {}
    for case in HOLES:
        for k, v in restated(case)[3].stats.items():
            if k != "areas2":  # the list of doubled areas
                follower[k] = follower.get(k, 0) + v
    assert all(follower.get(k, 0) > 0 for k in ("kept_outer", "kept_hole", "dropped_outer", "dropped_hole")), follower


# ---- the hard masks of tests/imbs_masks.py (what tests/test_gpu_22_imbs_area.py injects) -------------------------------------------------

@pytest.mark.parametrize("size", mk.SIZES + (mk.RECT_SIZE, (3, 3)), ids=lambda s: "%dx%d" % s)
def test_follower_form_equals_quad_form_on_the_hard_masks(size):
    """Every generator at minArea 0, 2.5, 30 and at two values taken from the mask itself: an area that occurs (kept: `area <
    minArea` is false) and that area plus one half (dropped), which puts the kept / dropped edge on exact halves."""
    H, W = size
    for name, m in mk.clip_masks(H, W):
        assert m.shape == (H, W) and m.dtype == bool
        assert name.startswith("rect") or 2 * int(m.sum()) <= H * W, name
        areas2 = im.area_filter_follower_many(m, [])[1]
        edge = mk.edge_min_area(areas2, H * W)
        min_areas = [0.0, 2.5, 30.0, edge, edge + 0.5]
        want, _ = im.area_filter_follower_many(m, min_areas)
        if H * W <= 33 * 70:  # the traced-once helper is the filter (the largest size would trace and fill everything twice for it)
            stats = {}
            assert np.array_equal(want[1], im.area_filter_follower(m, 2.5, stats)), name
            assert stats.get("areas2", []) == areas2
        at = [a for a in areas2 if a == int(2 * edge)]
        if any(0 < a / 2.0 < 0.6 * H * W for a in areas2):
            assert at and im.kept(at[0], edge, H * W) and not im.kept(at[0], edge + 0.5, H * W), (name, edge)
        for a, w in zip(min_areas, want):
            got = im.area_filter_quads(m, a)
            bad = np.argwhere(got != w)
            assert not len(bad), "%s %dx%d minArea %g: %d pixels differ, first at %s" % (name, H, W, a, len(bad), tuple(bad[0]))


@pytest.mark.parametrize("defect", ["zeros 8-connected", "ones 4-connected"])
def test_the_hard_masks_notice_a_wrong_connectivity(defect, monkeypatch):
    """The quad form with one labelling's connectivity swapped, at 33 x 70 and minArea 2.5: the corner-touching masks (ones that
    touch at a corner, holes that touch at a corner) and others tell it from the follower, so a device labelling with the wrong
    neighbourhood cannot pass tests/test_gpu_22_imbs_area.py."""
    label = im.label
    monkeypatch.setattr(im, "label", lambda m, conn8: label(m, defect == "zeros 8-connected"))
    caught = [name for name, m in mk.masks_for(33, 70) if not np.array_equal(im.area_filter_quads(m, 2.5), im.area_filter_follower(m, 2.5))]
    assert ("sieve" if defect == "zeros 8-connected" else "corners") in caught and len(caught) >= 3, caught


def _summed(stats):
    out = {}
    for st in stats:
        for k, v in st.items():
            if k != "areas2":
                out[k] = out.get(k, 0) + v
    return out


@pytest.mark.parametrize("size", mk.SIZES + (mk.RECT_SIZE,), ids=lambda s: "%dx%d" % s)
def test_injected_clips_hand_the_filter_the_painted_masks(size):
    """What tests/test_gpu_22_imbs_area.py relies on, from the restatement alone: the plane that reaches the area filter is the painted
    mask on every injected frame, `sudden_change` stays 0 (except after the rectangles), and the clips of one size take every branch."""
    H, W = size
    r = mk.reference(H, W)
    ctl = r["out"][2]
    assert len(r["planes"]) == len(r["masks"]) == len(mk.NAMES) + 2 * (size == mk.RECT_SIZE)
    for name, m, plane in zip(r["names"], r["masks"], r["planes"]):
        assert np.array_equal(plane, m), (name, int((plane != m).sum()))
    assert ctl[r["first"] - 1, 9] == 1 and not r["out"][0][:r["first"]].any()  # detecting before the first mask, and nothing found
    sudden = ctl[r["first"]:, 7]
    if size == mk.RECT_SIZE:  # both rectangles set more than half of the pixels; the next frame's changeBg sets bg_reset
        assert not sudden[:-2].any() and sudden[-2:].all() and ctl[-1, 6] == 1 and not ctl[:-1, 6].any()
        below, on = r["stats"][-2], r["stats"][-1]  # both sides of the 0.6 * numPixels edge
        assert below["areas2"] == [2 * 99] and below.get("kept_outer") == 1 and on["areas2"] == [2 * 108] and on.get("dropped_outer") == 1
        assert 0.6 * (H * W) == 108.0 and r["out"][0][-2].sum() == 255 * 120 and not r["out"][0][-1].any()
    else:
        assert not sudden.any()
    assert not (r["out"][0] == 180).any() and not (r["out"][0] == 80).any()  # the masks are the filter's output alone
    follower = _summed(r["stats"])
    assert all(follower.get(k, 0) > 0 for k in ("kept_outer", "kept_hole", "dropped_outer", "dropped_hole")), follower
    quads = _summed(mk.reference(H, W, quads=True)["stats"])
    assert np.array_equal(mk.reference(H, W, quads=True)["out"][0], r["out"][0])
    assert quads.get("chain", 0) > 0 and quads.get("dropped", 0) > 0, quads
    # a pixel survives on one of its component's own holes only where the component's outer border is dropped and a hole of it is
    # kept, that is where the outer area reaches 0.6 H W: at most (H - 3)(W - 3), so the five-pixel-wide frames cannot get there
    assert (quads.get("own_hole", 0) > 0) == ((H - 3) * (W - 3) >= 0.6 * H * W), quads
    if size == (65, 131):
        st = {name: mk.structure(m) for name, m in zip(r["names"], r["masks"])}
        assert st["checkerboard"]["holes"] >= 3000, st["checkerboard"]
        assert st["serpentine"]["spans"] >= 30 and (H * W + 255) // 256 == 34, st["serpentine"]  # one component through the workgroups' spans
        assert set(np.unique(im.label(r["masks"][r["names"].index("serpentine")], True))) == {-1, W + 1}  # a single component, named by its first pixel
        assert st["rings2"]["depth"] >= 8, st["rings2"]


def test_fixture_holds_every_case_and_is_small():
    path = os.path.join(im.GOLDEN, "imbs_ref.npz")
    assert os.path.getsize(path) <= 128 * 1024
    assert list(im.load()) == list(im.cases())  # no case was dropped by the poison runs
    for name, r in im.load().items():
        assert r["params"] == im.cases()[name], name


def test_fixture_conditions():
    got = im.load()
    with_label = {80: [], 180: []}
    for name, r in got.items():
        T, H, W = r["masks"].shape
        assert set(np.unique(r["masks"])) <= {0, 80, 180, 255}, name
        for v in with_label:
            if (r["masks"] == v).any():
                with_label[v].append(name)
        detects = r["control"][:, 9].any()
        if name == "default_short":
            assert not detects and not r["masks"].any() and r["control"][-1][3] > 0  # nothing builds; samples were taken
            continue
        assert detects, name
        if H * W > 35:
            assert any((m == 255).sum() >= 20 and (m == 0).sum() >= 20 for m in r["masks"]), name
    assert len(with_label[80]) >= 2 and len(with_label[180]) >= 2, with_label
    # the stories the cases are named for
    s = got["sudden"]["control"]
    assert s[:, 7].any() and {10.0, 3.0, 9.0} <= set(s[:, 4]) and s[-1][4] == 9.0 and 50.0 in set(s[:, 5])  # shrinks, restores inexactly
    p = got["persist"]["masks"][:, 7:12, 10:18]  # where the object stops, below the rows the moving one crosses (imbs_numpy.clip)
    seen180, seen255 = [(m == 180).sum() for m in p], [(m == 255).sum() for m in p]
    assert max(seen255) >= 30 and max(seen180) >= 30 and not p[-10:].any()  # foreground, then label 180, then past persistencePeriod: absorbed
    assert seen255.index(max(seen255)) < seen180.index(max(seen180))
    assert got["minbin1"]["control"][0][8] == 6 and got["minbin3"]["control"][0][8] == 2
    assert not got["tiny1x1"]["masks"].any() and not got["tiny3x3"]["masks"].any()  # the zero frame leaves at most one pixel
    full = got["full"]  # maxBgBins tall bins in front of another used one: the build loop leaves by `index == maxBgBins`, no isValid is cleared
    hit = (full["bins"][:, :4, 3] == [3, 3, 3, 1]).all(axis=1)
    assert hit.any() and full["control"][0][8] == 3 and (full["model"][hit][:, :, 3] == 1).all()


def test_hsv_gray_and_black_pixels():
    px = np.array([[60, 60, 60], [0, 0, 0], [255, 255, 255], [0, 0, 255], [0, 255, 0], [255, 0, 0], [10, 200, 90]], np.uint8)
    hsv = im.hsv_bytes(px)
    assert hsv[0].tolist() == [0, 0, 60] and hsv[1].tolist() == [0, 0, 0] and hsv[2].tolist() == [0, 0, 255]  # hue through 0 * inf = NaN -> 0
    assert hsv[3].tolist() == [0, 255, 255] and hsv[4].tolist() == [85, 255, 255] and hsv[5].tolist() == [170, 255, 255]


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------

def test_ids_and_struct_layout_match_c(tmp_path):
    inc = os.path.join(ROOT, "include")
    src = tmp_path / "imbs_abi.c"
    ids = ("34", "35", "BGS_IMBS", "BGS_ALGO_LAST", "(int)BGS_ALGO_LAST + 1")
    known = ", ".join("BGS_ALGO_KNOWN(%s)" % i for i in ids)
    offs = ", ".join("offsetof(bgs_imbs_params, %s)" % f for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bgs_hip.h"\nint main(){printf("%d %d %zu %d %d %d %d %zu' + " %d" * len(ids) + " %zu" * len(FIELDS)
                   + '\\n", (int)BGS_ALGO_LAST, (int)BGS_IMBS, sizeof(bgs_imbs_params), (int)BGS_IMBS_MAX_SAMPLES, (int)BGS_ALGO_COUNT, (int)BGS_ALGO_END, (int)BGS_ALGO_LIMIT, sizeof(bgs_params), '
                   + known + ", " + offs + ");return 0;}\n")
    exe = tmp_path / "imbs_abi"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(exe)], check=True)
    v = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert v[0] == capi.ALGO_LAST > capi.IMBS  # header and binding agree on the moving marker; its value is not pinned
    assert v[1] == 35 == capi.IMBS
    assert v[2] == C.sizeof(capi.BgsImbsParams) == 64 and v[3] == capi.IMBS_MAX_SAMPLES == 63
    assert v[4:7] == [21, 26, 28]  # the frozen markers
    assert v[7] == C.sizeof(capi.BgsParams) == 336  # bgs_params did not grow
    assert v[8:8 + len(ids)] == [1, 1, 1, 0, 0]  # one past the last id is unknown, symbolically
    assert v[8 + len(ids):] == [getattr(capi.BgsImbsParams, f).offset for f in FIELDS] == [0, 4, 8, 16, 20, 24, 28, 32, 36, 40, 44, 48, 56, 60]
    text = open(os.path.join(ROOT, "tracking_amd", "capi.py")).read()
    assert len(set(re.findall(r"^ALGO_LAST = (\d+)", text, re.M))) == 1


def test_unknown_ids_stay_unknown_and_the_new_one_is_known():
    p = capi.BgsParams()
    p.struct_size = C.sizeof(capi.BgsParams)
    for bad in (capi.ALGO_LAST, capi.ALGO_LAST + 1):
        assert capi.lib().bgs_default_params(bad, C.byref(p)) == capi.ERR_INVALID, bad
        h = C.c_void_p()
        assert capi.lib().bgs_create(bad, None, 0, 1, C.byref(h)) == capi.ERR_INVALID and b"unknown algorithm" in capi.lib().bgs_last_error()
    assert capi.lib().bgs_default_params(capi.IMBS, C.byref(p)) == capi.OK


def test_default_imbs_params():
    p = capi.imbs_default_params()
    assert p.struct_size == 64
    for k, v in im.DEFAULTS.items():
        want = float(np.float32(v)) if k in ("alpha", "beta") else v
        assert getattr(p, k) == want, k
    assert capi.lib().bgs_imbs_default_params(None) == capi.ERR_INVALID
    assert capi.imbs_default_params(numSamples=6).numSamples == 6


def test_every_refusal_names_the_class_and_needs_no_device():
    check = capi.lib().bgs_imbs_check
    name = im.CLASS_NAME.encode()
    assert check(None, 0, 0, 0) == capi.OK and check(None, 24, 32, 3) == capi.OK and check(None, 1, 1, 3) == capi.OK
    inf, nan = float("inf"), float("nan")
    bad = [dict(fps=0.0), dict(fps=-1.0), dict(fps=inf), dict(fps=nan), dict(minBinHeight=0), dict(numSamples=0), dict(numSamples=1), dict(numSamples=64), dict(numSamples=2, minBinHeight=3), dict(minBinHeight=31),
           dict(tau_s=-1), dict(tau_s=256), dict(tau_h=-1), dict(tau_h=256), dict(alpha=inf), dict(alpha=nan), dict(beta=inf), dict(beta=nan), dict(minArea=inf), dict(minArea=nan)]
    for kw in bad:
        assert check(C.byref(capi.imbs_default_params(**kw)), 0, 0, 0) == capi.ERR_UNSUPPORTED, kw
        assert name in capi.lib().bgs_last_error(), kw
    for kw in (dict(numSamples=2), dict(numSamples=63), dict(tau_s=0, tau_h=255), dict(minArea=0.0), dict(fps=0.001), dict(minBinHeight=1), dict(minBinHeight=30), dict(morphologicalFiltering=1)):
        assert check(C.byref(capi.imbs_default_params(**kw)), 0, 0, 0) == capi.OK, kw
    assert check(None, 24, 32, 1) == capi.ERR_UNSUPPORTED and name in capi.lib().bgs_last_error()  # gray frames
    assert check(C.byref(capi.imbs_default_params(struct_size=60)), 0, 0, 0) == capi.ERR_INVALID
    g = C.c_void_p()  # class groups: refused before any device is opened, the class named
    algos = (C.c_int * 2)(capi.FRAME_DIFF, capi.IMBS)
    assert capi.lib().bgs_group_create(algos, None, 2, 0, 1, C.byref(g)) == capi.ERR_UNSUPPORTED and name in capi.lib().bgs_last_error()


# ---- host layer ------------------------------------------------------------------------------------------------------------------------

def test_frame_processor_builds_the_class_and_writes_the_reference_xml(tmp_path):
    """Without a GPU the first frame ends in the one exception of the host layer; by then the class's banner is out and saveConfig()
    has written the reference's one key.  With a GPU the run succeeds."""
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    demo = os.path.join(ROOT, "tracking_amd", "lib", "bgs_demo")
    wd = str(tmp_path)
    os.makedirs(os.path.join(wd, "config"))
    raw = os.path.join(wd, "frames.raw")
    np.zeros((2, 8, 8, 3), np.uint8).tofile(raw)
    with open(os.path.join(wd, "config", "FrameProcessor.xml"), "w") as f:
        f.write('<?xml version="1.0"?>\n<opencv_storage>\n<enableFrameDifferenceBGS>0</enableFrameDifferenceBGS>\n<enableIMBS>1</enableIMBS>\n</opencv_storage>\n')
    r = subprocess.run([demo, raw, "8", "8", "2", os.path.join(wd, "out")], cwd=wd, capture_output=True, text=True)
    assert "IndependentMultimodalBGS()" in r.stdout, r.stdout + r.stderr
    assert r.returncode == 0 or "no HIP device" in r.stdout, r.stdout + r.stderr
    xml = open(os.path.join(wd, "config", "IndependentMultimodalBGS.xml")).read()
    assert xml == '<?xml version="1.0"?>\n<opencv_storage>\n<showOutput>1</showOutput>\n</opencv_storage>\n'
    assert "<enableIMBS>1</enableIMBS>" in open(os.path.join(wd, "config", "FrameProcessor.xml")).read()


def test_reference_side_adapters_compile_with_the_class(tmp_path):
    tu = tmp_path / "adapters_imbs.cpp"
    tu.write_text('#include "HipBGS.h"\n#include "HipFGDetector.h"\nIBGS* a() { return new hipbgs::IndependentMultimodalBGS; }\n')
    r = subprocess.run(["g++", "-std=gnu++0x", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "tests", "mock_opencv"), "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "tracking_amd", "host"), str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
