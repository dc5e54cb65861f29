"""The model stage of SJN_MultiCueBGS without a GPU: the numpy restatement (tests/multicue_numpy.py) against what
the reference's own, unmodified SJN_MultiCueBGS.cpp computed (tests/golden/multicue_ref.npz, made by tools/ref_fixtures/multicue),
bit for bit; the proof by enumeration that the XYZ bytes do not depend on a libm; the blur's integer taps; header, binding and
library agreement for the new symbols; every refusal of bgs_multicue_check."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import multicue_numpy as mc
import multicue_scenes as sc
from tracking_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgs_hip.h")


@pytest.mark.parametrize("case", mc.cases())
def test_restatement_matches_reference_fixture(case):
    r = mc.load()[case]
    p = r["params"]
    for d in range(len(r["update"])):  # step 1 of UpdateModel_Par, as the reference built it from the scripted boxes
        assert np.array_equal(r["update"][d], sc.update_map_of(r["boxes"][d], p["reduced_height"], p["reduced_width"])), d
    m, lms, confs = mc.run(p, r["frames"], r["ghost"], r["update"])
    assert np.array_equal(lms, r["landmark"])
    assert confs.tobytes() == r["conf"].tobytes()
    assert m.count == r["count"] == p["training_period"] + 2 and m.overflow == 0
    st = m.state()
    for k in mc.STATE_PLANES:
        assert mc.crc(st[k]) == r["plane_crc"][k], k
        if k in r["planes"]:
            assert st[k].tobytes() == r["planes"][k].tobytes(), k
    got = (int(m.tb.num.max()), int(m.tc.num.max()), int(m.cb.num.max()), int(m.cc.num.max()))
    assert all(g <= w for g, w in zip(got, r["maxima"]))  # the final books are no larger than the largest the reference reached on the way
    test_restatement_matches_reference_fixture.counts = getattr(test_restatement_matches_reference_fixture, "counts", {})
    test_restatement_matches_reference_fixture.counts[case] = dict(m.counts)


def test_fixture_reaches_every_branch():
    """The counters the generator stored: every listed branch is taken at least once, and the capacities are at least twice the
    largest book of each kind that the reference reached over the fixture (the drift scene included)."""
    f = mc.load()
    assert tuple(f["_counters"]) == mc.COUNTERS
    assert all(v > 0 for v in f["_counters"].values()), f["_counters"]
    slots = (mc.T_SLOTS, mc.TCACHE_SLOTS, mc.C_SLOTS, mc.CCACHE_SLOTS)
    assert all(2 * m <= s for m, s in zip(f["_maxima"], slots)), (f["_maxima"], slots)
    assert f["_maxima"][0] > 6 and f["_maxima"][2] > 10 and f["_maxima"][1] > 3 and f["_maxima"][3] > 3  # past the reference's initial array sizes
    per_case = getattr(test_restatement_matches_reference_fixture, "counts", {})
    if len(per_case) == len(mc.cases()):  # the whole module ran: the restatement's own counters add up to the stored ones
        for k in mc.COUNTERS:
            assert sum(c[k] for c in per_case.values()) == f["_counters"][k], k


def test_xyz_bytes_do_not_depend_on_libm():
    """All 2^24 BGR triples: no output byte changes when cos and sin move by 2 ulp either way (so neither by 1), except where the
    angle is 0 and both are exact.  The kernel's cos / sin and numpy's may therefore differ in the last place."""
    def moved(f, up):
        def g(h):
            v = f(h)
            w = np.nextafter(np.nextafter(v, np.inf if up else -np.inf), np.inf if up else -np.inf)
            return np.where(h == 0, v, w)
        return g
    g, r = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    tri = np.empty((256, 256, 3), np.uint8)
    tri[..., 1], tri[..., 2] = g, r
    changed = 0
    for b in range(256):
        tri[..., 0] = b
        base = mc.xyz_of(tri)
        for up in (False, True):
            changed += int((mc.xyz_of(tri, moved(np.cos, up), moved(np.sin, up)) != base).sum())
    assert changed == 0


def test_xyz_known_values():
    bgr = np.array([[0, 0, 0], [255, 255, 255], [0, 0, 255], [0, 255, 0], [255, 0, 0], [10, 10, 10]], np.uint8)
    out = mc.xyz_of(bgr)
    assert out[0].tolist() == [127, 127, 0] and out[1].tolist() == [127, 127, 255] and out[5].tolist() == [127, 127, 10]
    assert out[2].tolist() == [255, 127, 255]  # pure red: H = 0, cos = 1, sin = 0
    assert out[3, 2] == 255 and out[4, 2] == 255 and out[3, 0] < 127 and out[4, 0] < 127


def test_integer_taps():
    assert mc.integer_taps(7, 0.7) == (0, 2, 53, 146, 53, 2, 0) == mc.TAPS
    assert sum(mc.TAPS) == 256
    img = np.full((5, 6, 3), 77, np.uint8)
    assert (mc.blur7(img) == 77).all()  # taps that sum to 256 leave a flat image as it is, reflected borders included


def test_reduce_indices():
    f = np.arange(7 * 9 * 3, dtype=np.uint8).reshape(7, 9, 3)
    out = mc.reduce_frame(f, 12, 16)  # a frame smaller than the reduced size repeats pixels
    assert out.shape == (12, 16, 3) and np.array_equal(out[11, 15], f[int(11 * (7 / 12)), int(15 * (9 / 16))])
    assert np.array_equal(mc.reduce_frame(f, 7, 9), f)


def test_header_binding_and_library_agree(tmp_path):
    h = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = ["bgs_multicue_default_params", "bgs_multicue_check", "bgs_multicue_create", "bgs_multicue_destroy", "bgs_multicue_train_device",
             "bgs_multicue_landmark_device", "bgs_multicue_update_device", "bgs_multicue_get_state", "bgs_multicue_xyz_device"]
    lib = C.CDLL(capi.LIB_PATH)
    bound = {n for n, _, _ in capi.SYMBOLS}
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, h), n
        assert hasattr(lib, n) and n in bound, n
    for macro, want in (("TEXTURE", mc.T_SLOTS), ("TEXTURE_CACHE", mc.TCACHE_SLOTS), ("COLOR", mc.C_SLOTS), ("COLOR_CACHE", mc.CCACHE_SLOTS)):
        m = re.search(r"#define BGS_MULTICUE_%s_SLOTS (\d+)" % macro, h)
        assert m and int(m.group(1)) == want == getattr(capi, "MULTICUE_%s_SLOTS" % macro), macro
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bgs_hip.h"\nint main(){printf("%zu %zu %zu\\n", sizeof(bgs_multicue_params), '
                   'offsetof(bgs_multicue_params, learning_rate), offsetof(bgs_multicue_params, cache_clear_period));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, lr, last = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    P = capi.BgsMulticueParams
    assert size == C.sizeof(P) and lr == P.learning_rate.offset and last == P.cache_clear_period.offset
    p = capi.multicue_default_params()
    assert p.struct_size == size
    assert {k: getattr(p, k) for k in mc.INT_FIELDS} == {k: mc.DEFAULTS[k] for k in mc.INT_FIELDS}
    assert np.float32(p.learning_rate) == np.float32(mc.DEFAULTS["learning_rate"])
    assert capi.lib().bgs_abi_version() == 1 and capi.ALGO_LAST == 37  # no class id yet


def test_every_refusal_without_a_device():
    chk = capi.lib().bgs_multicue_check

    def rc(rows=0, cols=0, **kw):
        return chk(C.byref(capi.multicue_default_params(**kw)), rows, cols)

    assert chk(None, 0, 0) == capi.OK and rc() == capi.OK and rc(1080, 1920) == capi.OK and rc(7, 9) == capi.OK
    for k in ("training_period", "absorption_period", "back_clear_period", "cache_clear_period"):
        for v in (0, -1, 32768):
            assert rc(**{k: v}) == capi.ERR_UNSUPPORTED, (k, v)
            assert "SJN_MultiCueBGS" in capi.last_error() and k in capi.last_error()
        assert rc(**{k: 1}) == capi.OK and rc(**{k: 32767}) == capi.OK
    for k in ("texture_train_vol_range", "color_train_vol_range"):
        for v in (-1, 32768):
            assert rc(**{k: v}) == capi.ERR_UNSUPPORTED, (k, v)
            assert "SJN_MultiCueBGS" in capi.last_error() and k in capi.last_error()
        assert rc(**{k: 0}) == capi.OK and rc(**{k: 32767}) == capi.OK
    for v in (float("nan"), float("inf"), float("-inf")):
        assert rc(learning_rate=v) == capi.ERR_UNSUPPORTED and "SJN_MultiCueBGS" in capi.last_error()
    assert rc(reduced_width=4) == capi.ERR_UNSUPPORTED and rc(reduced_height=4) == capi.ERR_UNSUPPORTED and "SJN_MultiCueBGS" in capi.last_error()
    assert rc(reduced_width=5, reduced_height=5) == capi.OK
    assert rc(reduced_width=161, reduced_height=128) == capi.ERR_UNSUPPORTED and "BGS_CANNY_MAX_PIXELS" in capi.last_error()
    assert rc(reduced_width=160, reduced_height=128) == capi.OK  # exactly BGS_CANNY_MAX_PIXELS
    p = capi.multicue_default_params()
    p.struct_size = 8
    assert chk(C.byref(p), 0, 0) == capi.ERR_INVALID and "struct_size" in capi.last_error()
    h = C.c_void_p()
    assert capi.lib().bgs_multicue_create(0, 1, C.byref(capi.multicue_default_params(reduced_width=3)), C.byref(h)) == capi.ERR_UNSUPPORTED and not h.value
    assert capi.lib().bgs_multicue_create(0, 0, None, C.byref(h)) == capi.ERR_INVALID and not h.value
