"""The box stage and the whole-frame step of SJN_MultiCueBGS without a GPU: the numpy restatement
(tests/multicue_box_numpy.py) against what the reference's own, unmodified SJN_MultiCueBGS.cpp computed
(tests/golden/multicue_box_ref.npz, made by tools/ref_fixtures/multicue), byte for byte; the count-based ghost test against the
reference's recorded distance on every box; hand-derived labelling patterns; header, binding and library agreement for the new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import multicue_box_numpy as mb
import multicue_numpy as mc
from tracking_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgs_hip.h")
FIX = mb.load()


def same_frame(r, want_maps, want_boxes, where):
    assert r["count"] == len(want_boxes) <= mb.MAX_BOXES and r["box_overflow"] == 0, where
    assert np.array_equal(r["fore"] != 0, want_maps[0] != 0) and set(np.unique(r["fore"])) <= {0, 255}, (where, "fore")
    assert np.array_equal(r["ghost"], want_maps[1]), (where, "ghost")
    assert np.array_equal(r["update"], want_maps[2]), (where, "update")
    assert np.array_equal(r["boxes"], want_boxes), (where, "boxes")


@pytest.mark.parametrize("case", list(FIX["post"]))
def test_box_stage_matches_reference_fixture(case):
    f = FIX["post"][case]
    windows = []
    r = mb.boxes(f["landmark"], f["frame"], windows)
    same_frame(r, (f["fore"], f["ghost"], f["update"]), f["boxes"], case)
    at = 0
    for k, q in enumerate(f["boxes"]):  # the reference's own CalculateHausdorffDist on every box that passed the size test
        if not q[8]:
            assert f["dist"][k] == -1
            continue
        gw, ea, fw, eb = windows[at]
        at += 1
        assert mb.hausdorff(ea, eb) == f["dist"][k], (case, k)
    assert at == len(windows)


@pytest.mark.parametrize("case", list(FIX["step"]))
def test_whole_step_matches_reference_fixture(case):
    f = FIX["step"][case]
    step = mb.Step(f["params"])
    for t, frame in enumerate(f["frames"]):
        img = step.process(frame)
        assert mc.crc(img) == f["image_crc"][t], (case, t)
        if f["images"] is not None:
            assert np.array_equal(img, f["images"][t]), (case, t)
        if t < f["train"]:
            assert not img.any()
            continue
        d = t - f["train"]
        same_frame(step.last, (f["fore"][d], f["ghost"][d], f["update"][d]), f["boxes"][d], (case, d))
    st = step.m.state()
    for k in mc.STATE_PLANES:
        assert mc.crc(st[k]) == f["plane_crc"][k], (case, k)
    assert step.m.overflow == 0 and step.box_overflow == 0 and step.m.count == f["params"]["training_period"] + 2


def test_count_based_ghost_test_equals_the_reference_distance():
    """Every box of the fixture that passed the size test: `near <= (int)(0.9 n)` (what the device decides by) against the double
    the reference's CalculateHausdorffDist returned, and the final m_ValidBox against both."""
    seen = 0
    sets = [(f["boxes"], f["dist"]) for f in FIX["post"].values()]
    sets += [(b, d) for f in FIX["step"].values() for b, d in zip(f["boxes"], f["dist"])]
    for boxes, dist in sets:
        for q, dd in zip(boxes, dist):
            if not q[8]:
                assert not q[9] and not q[10:13].any()
                continue
            seen += 1
            assert mb.ghost_by_count(int(q[10]), int(q[11]), int(q[12])) == (dd > 10) == (not q[9]), (q, dd)
    assert seen > 100


def test_fixture_reaches_every_branch():
    assert all(v > 0 for v in FIX["branches"].values()), FIX["branches"]
    assert max(len(f["boxes"]) for f in FIX["post"].values()) == mb.MAX_BOXES  # exactly full, never over


def pattern(rows):
    return np.array([[255 if c == "X" else 0 for c in r] for r in rows], np.uint8)


def test_labelling_u_shape():
    lab, n, st = mb.labeling(pattern([".....", ".X.X.", ".X.X.", ".XXX.", "....."]))
    assert n == 1 and st["pass1_labels"] == 2 and st["merges"] == 1
    assert lab.tolist() == [[0, 0, 0, 0, 0], [0, 1, 0, 1, 0], [0, 1, 0, 1, 0], [0, 1, 1, 1, 0], [0, 0, 0, 0, 0]]


def test_labelling_staircase_ends_with_two_labels_for_one_blob():
    """Label 3 is copied from 2 (aTable1[3] = 2) and then from 1; nobody sends 2 to 1, so the step on the right keeps its own label."""
    fore = pattern(["........", ".X....X.", ".X..XXX.", ".XXXX...", "........"])
    lab, n, st = mb.labeling(fore)
    assert n == 2 and st["pass1_labels"] == 3 and st["merges"] == 2
    assert lab.tolist() == [[0] * 8, [0, 1, 0, 0, 0, 0, 2, 0], [0, 1, 0, 0, 1, 1, 2, 0], [0, 1, 1, 1, 1, 0, 0, 0], [0] * 8]
    assert mb.blobs4(fore)[1] == 1


def test_labelling_comb_with_chained_merges():
    """aTable1[3] = aTable1[2] happens while aTable1[2] is still 2; aTable1[2] = 1 comes later and is never passed on."""
    fore = pattern([".......", ".....X.", "...X.X.", ".X.X.X.", ".XXXXX.", "......."])
    lab, n, st = mb.labeling(fore)
    assert n == 2 and st["pass1_labels"] == 3 and st["merges"] == 2
    assert lab.tolist() == [[0] * 7, [0, 0, 0, 0, 0, 1, 0], [0, 0, 0, 1, 0, 1, 0], [0, 2, 0, 1, 0, 1, 0], [0, 2, 2, 1, 1, 1, 0], [0] * 7]
    assert mb.blobs4(fore)[1] == 1


def test_majority_counts_only_255():
    lm = np.zeros((9, 9), np.uint8)
    lm[2:7, 2:7] = 125
    assert not mb.majority(lm).any()  # 125 counts as 0
    lm[2:5, 2:6] = 255  # 12 pixels
    got = mb.majority(lm)
    assert got[3, 3] == 255 and got[3, 4] == 255 and got[2, 3] == 255 and got[5, 3] == 0 and not got[:2].any() and not got[:, :2].any()


def test_two_nearest_neighbour_rules_differ():
    """A 39 x 52 frame at 160 x 120: row 40 and column 40 read source 13 in ReduceImageSize and 12 in cvResize(CV_INTER_NN)."""
    frame = np.zeros((39, 52, 3), np.uint8)
    frame[..., 0] = np.arange(39)[:, None]
    frame[..., 1] = np.arange(52)[None, :]
    red, (nn, sy, sx) = mc.reduce_frame(frame, 120, 160), mb.resize_nn(frame, 120, 160)
    assert red[40, 0, 0] == 13 and nn[40, 0, 0] == 12 == sy[40] and red[0, 40, 1] == 13 and nn[0, 40, 1] == 12 == sx[40]


def test_bilinear_identity_and_half():
    rng = np.random.RandomState(5)
    a = rng.randint(0, 256, (12, 16)).astype(np.uint8)
    assert np.array_equal(mb.resize_linear(a, 12, 16), a)
    s = a.astype(np.int64)
    assert np.array_equal(mb.resize_linear(a, 6, 8), ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8))
    up = mb.resize_linear(np.array([[0, 255]] * 2, np.uint8), 2, 8)
    assert up[0, 0] == 0 and up[0, -1] == 255 and (np.diff(up[0].astype(int)) >= 0).all() and 0 < up[0, 3] < 255  # values in between are kept


def test_header_binding_and_library_agree():
    h = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = C.CDLL(capi.LIB_PATH)
    bound = {n: a for n, _, a in capi.SYMBOLS}
    for n, nargs in (("bgs_multicue_boxes_device", 11), ("bgs_multicue_process_device", 6)):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % n, h)
        assert m and len(m.group(1).split(",")) == nargs == len(bound[n]), n
        assert hasattr(lib, n), n
    for macro, want in (("MAX_BOXES", mb.MAX_BOXES), ("BOX_FIELDS", len(mb.BOX_FIELDS))):
        m = re.search(r"#define BGS_MULTICUE_%s (\d+)" % macro, h)
        assert m and int(m.group(1)) == want == getattr(capi, "MULTICUE_" + macro), macro
    assert capi.lib().bgs_abi_version() == 1 and capi.ALGO_LAST == 37  # still no class id
