"""T2FGMM_UM / T2FGMM_UV (USTC_BGS types 17 and 18) without a GPU: the numpy restatement against the fixture made from the reference's
own tb/T2FGMM.cpp, what each fixture case covers, the C ABI (ids, the third hole, bgs_t2f_params, the refusals) and the host layer
(class list, XML keys and defaults, the type table, the reference-side adapters)."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import t2f_numpy as tn
from tracking_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "tracking_amd", "host")
ALL = [(typ, case) for typ in tn.TYPES for case in tn.cases()]
SIZEOF_BGS_PARAMS_PARENT = 336
T2F_FIELDS = ["struct_size", "threshold", "alpha", "km", "kv", "gaussians"]


@functools.lru_cache(maxsize=None)
def restated(typ, case):
    r = tn.load()[typ, case]
    return tn.run(typ, r["params"], r["frames"])


# ---- the restatement and the fixture -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("typ,case", ALL, ids=["%s-%s" % tc for tc in ALL])
def test_restatement_equals_the_reference_fixture_bit_for_bit(typ, case):
    r = tn.load()[typ, case]
    masks, mdl = restated(typ, case)
    assert np.array_equal(masks, r["masks"]), int((masks != r["masks"]).sum())
    n = masks.shape[1] * masks.shape[2]
    assert ("modes" in r) == (n <= tn.PLANE_PIXELS)
    if "modes" in r:
        K = r["params"]["gaussians"]
        assert np.array_equal(mdl.count, r["nmodes"])
        below = tn.below_count(None, r["nmodes"], K).reshape(K * tn.FIELDS, n)
        assert below.any()
        assert np.array_equal(mdl.planes().view(np.uint32)[below], r["modes"].view(np.uint32)[below])


def test_fixture_holds_every_case_for_both_types_and_is_small():
    assert os.path.getsize(os.path.join(tn.dp_ref.GOLDEN, "t2f_ref.npz")) <= 128 * 1024
    assert sorted(tn.load()) == sorted(ALL)
    assert list(tn.cases()) == ["default", "tile", "ragged", "ragged_o1", "ragged_o2", "tiny5x7", "tiny1x1", "modes_k1", "modes_k2", "modes_k4", "modes_k5",
                                "thr2_km3_kv03", "alpha05", "ties"]
    shapes = {case: tn.load()["um", case]["masks"].shape[1:] for case in tn.cases()}
    assert shapes["default"] == (80, 96) and shapes["tile"] == (16, 64) and shapes["ragged"] == shapes["ragged_o1"] == shapes["ragged_o2"] == (37, 53)
    assert shapes["tiny5x7"] == (5, 7) and shapes["tiny1x1"] == (1, 1)
    c = tn.cases()
    assert c["default"] == dict(tn.DEFAULTS, input="frames_96x80") and tn.DEFAULTS == dict(threshold=9.0, alpha=0.01, km=1.5, kv=float(np.float32(0.6)), gaussians=3)
    assert c["ragged"]["input"] == c["ragged_o1"]["input"] == c["ragged_o2"]["input"]  # one seeded clip, entered 0, 1 and 2 frames late
    assert [c[k]["window"][0] for k in ("ragged", "ragged_o1", "ragged_o2")] == [0, 1, 2]
    whole = tn.frames_of(dict(c["ragged"], window=[0, 17]))
    for k, o in (("ragged", 0), ("ragged_o1", 1), ("ragged_o2", 2)):
        assert np.array_equal(tn.load()["um", k]["frames"], whole[o:o + 15])
    env = tn.environment()  # the build-environment answers the bits depend on
    assert env["sqrt_overload"] == "sqrt(float) -> float" and "equal keys keep their order" in env["qsort"] and len(env["poison_bytes"]) == 2
    assert "-ffp-contract=off" in env["flags"] and "T2FGMM.cpp" in env["sources"] and "Image.cpp" in env["sources"]


@pytest.mark.parametrize("typ", tn.TYPES)
def test_each_case_covers_what_it_claims(typ):
    cases = tn.load()
    for K in (1, 2, 4, 5):
        r = cases[typ, "modes_k%d" % K]
        assert r["params"]["gaussians"] == K and int((r["nmodes"] == K).sum()) > 0 and int(r["nmodes"].max()) == K, K
    assert int((cases[typ, "default"]["masks"].reshape(24, -1)[1:] != 0).sum()) > 0
    assert restated(typ, "ties")[1].ties > 0  # equal `significants` met the sort: the stable order decided
    assert cases[typ, "ties"]["params"]["alpha"] == float(np.float32(1e-8)) and set(np.unique(cases[typ, "ties"]["frames"])) == {0, 128, 255}
    p = cases[typ, "thr2_km3_kv03"]["params"]
    assert (p["threshold"], p["km"], p["kv"]) == (2.0, 3.0, float(np.float32(0.3)))
    assert cases[typ, "alpha05"]["params"]["alpha"] == 0.5
    if typ == "um":  # both branches of the interval test, on modes that were tried
        m = restated(typ, "thr2_km3_kv03")[1]
        assert m.um_inside > 100 and m.um_outside > 100, (m.um_inside, m.um_outside)
    for case in tn.cases():  # no case passes on an all-one-value mask
        m = cases[typ, case]["masks"]
        if m.shape[1] * m.shape[2] > 35:
            fg = (m[1:] != 0).reshape(len(m) - 1, -1).sum(1)
            bg = m.shape[1] * m.shape[2] - fg
            assert ((fg >= 20) & (bg >= 20)).any(), (typ, case, fg.tolist())


def test_the_mean_only_moves_down():
    """mu -= k * |d|: the reference's behaviour, pinned by the fixture.  A mode that keeps matching a brighter pixel walks away from
    it; no matched update ever raises a mean."""
    m = tn.T2FGMM(tn.UM, 1)
    m.step(np.array([[100, 100, 100]], np.uint8))
    before = m.modes[0, tn.MU:tn.MU + 3, 0].copy()
    m.step(np.array([[110, 90, 100]], np.uint8))
    after = m.modes[0, tn.MU:tn.MU + 3, 0]
    assert m.count[0] == 1 and after[0] < before[0] and after[1] < before[1] and after[2] == before[2]
    assert tn.load()["um", "default"]["masks"].shape[0] == 24 and restated("um", "default")[1].modes[:, tn.MU:tn.MU + 3].min() < -1000


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------

def test_ids_third_hole_and_struct_layout_match_c(tmp_path):
    inc = os.path.join(ROOT, "include")
    src = tmp_path / "t2f_abi.c"
    ids = ("-1", "30", "31", "32", "33", "BGS_ALGO_LAST", "(int)BGS_ALGO_LAST + 1", "BGS_T2FGMM_UM", "BGS_T2FGMM_UV")
    known = ", ".join("BGS_ALGO_KNOWN(%s)" % i for i in ids)
    offs = ", ".join("offsetof(bgs_t2f_params, %s)" % f for f in T2F_FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bgs_hip.h"\nint main(){printf("%d %zu %zu %d %d %d %d %d' + " %d" * len(ids) + " %zu" * len(T2F_FIELDS)
                   + '\\n", (int)BGS_ALGO_LAST, sizeof(bgs_params), sizeof(bgs_t2f_params), (int)BGS_ALGO_COUNT, (int)BGS_ALGO_END, (int)BGS_ALGO_LIMIT, (int)BGS_T2FGMM_UM, (int)BGS_T2FGMM_UV, '
                   + known + ", " + offs + ");return 0;}\n")
    exe = tmp_path / "t2f_abi"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(exe)], check=True)
    v = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    last, v = v[0], v[1:]
    assert last == capi.ALGO_LAST > capi.T2FGMM_UV  # header and binding agree on the moving marker; its value is not pinned
    assert v[0] == SIZEOF_BGS_PARAMS_PARENT == C.sizeof(capi.BgsParams)  # bgs_params did not grow
    assert v[1] == C.sizeof(capi.BgsT2fParams) == 40
    assert v[2:5] == [21, 26, 28]  # the frozen markers
    assert v[5:7] == [32, 33] == [capi.T2FGMM_UM, capi.T2FGMM_UV]
    assert v[7:7 + len(ids)] == [0, 1, 0, 1, 1, 0, 0, 1, 1]  # 31 is the third hole; one past the last id is unknown, symbolically
    assert v[7 + len(ids):] == [getattr(capi.BgsT2fParams, f).offset for f in T2F_FIELDS] == [0, 8, 16, 24, 28, 32]
    text = open(os.path.join(ROOT, "tracking_amd", "capi.py")).read()
    assert len(set(re.findall(r"^ALGO_LAST = (\d+)", text, re.M))) == 1  # the constant appears twice in capi.py: one value


def test_unknown_ids_stay_unknown():
    p = capi.BgsParams()
    p.struct_size = C.sizeof(capi.BgsParams)
    for bad in (31, capi.ALGO_LAST, capi.ALGO_LAST + 1):
        assert capi.lib().bgs_default_params(bad, C.byref(p)) == capi.ERR_INVALID, bad
        h = C.c_void_p()
        assert capi.lib().bgs_create(bad, None, 0, 1, C.byref(h)) == capi.ERR_INVALID and b"unknown algorithm" in capi.lib().bgs_last_error()
    for ok in (capi.T2FGMM_UM, capi.T2FGMM_UV):
        assert capi.lib().bgs_default_params(ok, C.byref(p)) == capi.OK


def test_default_t2f_params():
    p = capi.t2f_default_params()
    assert (p.struct_size, p.threshold, p.alpha, p.km, p.kv, p.gaussians) == (40, 9.0, 0.01, 1.5, np.float32(0.6), 3)
    d = tn.DEFAULTS
    assert (p.threshold, p.alpha, p.km, p.kv, p.gaussians) == (d["threshold"], d["alpha"], d["km"], d["kv"], d["gaussians"])
    assert capi.lib().bgs_t2f_default_params(None) == capi.ERR_INVALID
    assert capi.t2f_default_params(gaussians=5).gaussians == 5


@pytest.mark.parametrize("algo,name", [(capi.T2FGMM_UM, b"T2FGMM_UM"), (capi.T2FGMM_UV, b"T2FGMM_UV")])
def test_every_refusal_names_the_class_and_needs_no_device(algo, name):
    check = capi.lib().bgs_t2f_check
    assert check(algo, None, 0, 0, 0) == capi.OK and check(algo, None, 80, 96, 3) == capi.OK and check(algo, None, 1, 1, 3) == capi.OK
    bad = [dict(gaussians=0), dict(gaussians=6), dict(gaussians=-1), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(threshold=1e300),
           dict(alpha=float("nan")), dict(alpha=float("-inf")), dict(alpha=1.0), dict(alpha=1.5), dict(alpha=-0.01), dict(km=float("inf")), dict(km=float("nan")), dict(kv=float("nan")), dict(kv=float("inf"))]
    if algo == capi.T2FGMM_UV:
        bad.append(dict(kv=0.0))
    for kw in bad:
        p = capi.t2f_default_params(**kw)
        assert check(algo, C.byref(p), 0, 0, 0) == capi.ERR_UNSUPPORTED, kw
        assert name in capi.lib().bgs_last_error(), kw
    if algo == capi.T2FGMM_UM:  # kv does not enter UM's distance
        assert check(algo, C.byref(capi.t2f_default_params(kv=0.0)), 0, 0, 0) == capi.OK
    for K in (1, 2, 3, 4, 5):
        assert check(algo, C.byref(capi.t2f_default_params(gaussians=K)), 0, 0, 0) == capi.OK
    for a in (0.0, 1e-8, 0.5, float(np.nextafter(np.float32(1), np.float32(0)))):
        assert check(algo, C.byref(capi.t2f_default_params(alpha=a)), 0, 0, 0) == capi.OK, a
    assert check(algo, None, 80, 96, 1) == capi.ERR_UNSUPPORTED and name in capi.lib().bgs_last_error()  # gray frames
    assert check(algo, C.byref(capi.t2f_default_params(struct_size=32)), 0, 0, 0) == capi.ERR_INVALID
    assert check(capi.DP_GRIMSON_GMM, None, 0, 0, 0) == capi.ERR_INVALID
    g = C.c_void_p()  # class groups: refused before any device is opened, the class named
    algos = (C.c_int * 2)(capi.FRAME_DIFF, algo)
    assert capi.lib().bgs_group_create(algos, None, 2, 0, 1, C.byref(g)) == capi.ERR_UNSUPPORTED and name in capi.lib().bgs_last_error()


# ---- host layer ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def demo():
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    return os.path.join(ROOT, "tracking_amd", "lib", "bgs_demo")


def run_ustc(demo, wd, utype):
    os.makedirs(os.path.join(wd, "config"), exist_ok=True)
    raw = os.path.join(wd, "frames.raw")
    np.zeros((2, 8, 8, 3), np.uint8).tofile(raw)
    return subprocess.run([demo, raw, "8", "8", "2", os.path.join(wd, "out"), str(utype)], cwd=wd, capture_output=True, text=True)


@pytest.mark.parametrize("utype", [15, 19, 20, 23, 30, 33, 34])
def test_the_seven_types_without_a_class_still_throw(demo, tmp_path, utype):
    """What `i == 17)` not occurring in the type table protected: no type silently runs another class.  Kept at run time: USTC_BGS of
    every type that has no class here throws BGS_ERR_UNSUPPORTED at construction, before any class banner and any device."""
    r = run_ustc(demo, str(tmp_path), utype)
    assert r.returncode == 1 and "USTC_BGS: type %d is outside the package_bgs hot path" % utype in r.stdout, r.stdout
    assert "()" not in r.stdout.replace("std::exception", "")  # no constructor banner: nothing was built


@pytest.mark.parametrize("utype,name", [(17, "T2FGMM_UM"), (18, "T2FGMM_UV")])
def test_types_17_and_18_build_their_own_class_and_write_the_reference_xml(demo, tmp_path, utype, name):
    """Without a GPU the first frame ends in the one exception of the host layer; by then the class's banner is out and saveConfig()
    has written the reference's keys in the reference's order with the reference's defaults.  With a GPU the run succeeds."""
    r = run_ustc(demo, str(tmp_path), utype)
    assert name + "()" in r.stdout and r.stdout.count("()") - r.stdout.count("~") <= 1, r.stdout
    assert r.returncode == 0 or "no HIP device" in r.stdout, r.stdout
    xml = (tmp_path / "config" / (name + ".xml")).read_text()
    assert xml == ('<?xml version="1.0"?>\n<opencv_storage>\n<threshold>9.</threshold>\n<alpha>0.01</alpha>\n<km>1.5</km>\n<kv>%s</kv>\n<gaussians>3</gaussians>\n'
                   "<showOutput>1</showOutput>\n</opencv_storage>\n" % ("%.16g" % float(np.float32(0.6))))


def test_reference_side_adapters_compile_with_the_t2f_classes(tmp_path):
    tu = tmp_path / "adapters_t2f.cpp"
    tu.write_text('#include "HipBGS.h"\n#include "HipFGDetector.h"\nIBGS* a() { return new hipbgs::T2FGMM_UM; }\nIBGS* b() { return new hipbgs::T2FGMM_UV; }\n'
                  "CvFGDetector* c() { return new HipFGDetector(17); }\nCvFGDetector* d() { return new HipFGDetector(18); }\n")
    r = subprocess.run(["g++", "-std=gnu++0x", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "tests", "mock_opencv"), "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "tracking_amd", "host"), str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
