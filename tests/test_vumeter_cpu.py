"""VuMeter (BGS_VUMETER, USTC_BGS type 31) on the CPU: the numpy restatement (tests/vumeter_numpy.py) against the outputs of the
reference's own model code (tests/golden/vumeter_ref.npz: av/TBackground.cpp and av/TBackgroundVuMeter.cpp compiled unmodified
behind a stand-in OpenCV header whose cvConvertScale works in float), what the fixtures claim to cover, the gray
formula, the C ABI (ids, struct tail, defaults, setter rules) and the host class list."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import vumeter_numpy as vn
from tracking_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
CASES = ["default", "bins3", "bins100", "bins200", "bins1", "setters", "thr_edge", "denormal", "denormal_mid", "long"]
WHOLE_MODEL = ["bins3", "bins1", "denormal", "denormal_mid", "long"]  # the cases that hold every histogram plane after the last frame
VU_FIELDS = ["vu_bin_size", "vu_enable_filter", "vu_alpha", "vu_threshold"]
# the `denormal` case, determined with the restatement: every pixel's first bin is last hit on frame 2 (0-based), is an f32 denormal
# after the decay of frames 125..146 (22 frames) and exactly 0 from frame 147 on
DENORMAL_FIRST, DENORMAL_LAST, ZERO_FROM = 125, 146, 147

_Z = None


def golden(case):
    """(record, model keyword parameters, gray input frames) of one fixture case; the input is checked against its CRC-32 first."""
    global _Z
    if _Z is None:
        _Z = dict(np.load(os.path.join(GOLDEN, "vumeter_ref.npz")))
    r = {k.split("/", 1)[1]: v for k, v in _Z.items() if k.startswith(case + "/")}
    p = json.loads(str(r["params"]))
    frames = vn.clip(p.pop("input"))
    assert vn.crc(frames) == int(r["input_crc32"]), "%s: input clip differs from the one the fixture was made from" % case
    return r, p, frames


def masks_of(r):
    T, rows, cols = (int(v) for v in r["shape"])
    return np.unpackbits(r["masks"], axis=-1)[..., :cols].reshape(T, rows, cols) * np.uint8(255)


def run_restatement(case, watch=None):
    r, p, frames = golden(case)
    m = vn.Model(**p)
    bg = frames[0].copy()
    want = masks_of(r)
    bad_bits = bad_bg = 0
    for t, g in enumerate(frames):
        mask = m.update(g, bg)
        bad_bits += int((mask != want[t]).sum())
        bad_bg += int(vn.crc(bg) != int(r["bg_crc32"][t]))
        if watch:
            watch(t, m)
    return m, bg, bad_bits, bad_bg, r


@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_reference_fixture_bit_for_bit(case):
    m, bg, bad_bits, bad_bg, r = run_restatement(case)
    assert (bad_bits, bad_bg) == (0, 0)
    assert np.array_equal(bg, r["bg_last"]) and m.count == int(r["count"][0]) == len(masks_of(r))
    assert ("hist" in r) == (case in WHOLE_MODEL)
    if case in WHOLE_MODEL:
        assert m.hist.shape == r["hist"].shape and np.array_equal(m.hist.view(np.uint32), r["hist"].view(np.uint32))


def test_fixtures_cover_what_they_claim():
    for case in CASES:
        r, p, frames = golden(case)
        masks = masks_of(r)
        assert set(np.unique(masks)) == {0, 255}, case                 # both mask values
        assert not masks[:vn.QUIET_FRAMES].any() and masks[vn.QUIET_FRAMES:].any(), case  # m_nCount < 5
    assert golden("default")[1] == {} and len(golden("long")[2]) >= 200
    for case, bins, wraps in (("bins3", 85, 255), ("bins100", 2, 200), ("bins200", 1, 200), ("bins1", 256, None)):
        r, p, frames = golden(case)
        m = vn.Model(**p)
        assert m.bin_count == bins, case
        if wraps is not None:  # bytes whose index is >= binCount occur and land in bin 0
            hit = frames >= wraps
            assert hit.any() and (frames // m.bin_size >= bins)[hit].all() and (m.bins(frames)[hit] == 0).all(), case
    assert (golden("bins3")[2] == 255).any()
    r, p, frames = golden("setters")
    m = vn.Model(**p)
    assert p == dict(bin_size=0, alpha=1.5, threshold=0.0) and (m.bin_size, m.alpha, m.threshold) == (8, 0.995, 0.03)
    for case in ("long", "default", "thr_edge"):
        assert run_restatement(case)[0].replaced > 100, case  # backgrounds are replaced
    # thr_edge: after the quiet frames some pixel's mask goes 255 -> 0 (its bin rose through the threshold) and later 0 -> 255
    # (it left, the bin decayed below the threshold, it came back)
    mk = masks_of(golden("thr_edge")[0])[vn.QUIET_FRAMES:].astype(np.int16)
    d = np.diff(mk, axis=0)
    fell = np.cumsum(d < 0, axis=0) > 0
    assert ((d > 0)[1:] & fell[:-1]).any()


def test_the_denormal_case_passes_through_denormals_and_ends_at_zero():
    r, p, frames = golden("denormal")
    assert p["alpha"] < 0.5 and np.log2(p["alpha"]) % 1 != 0  # below 1/2 the smallest denormal rounds to 0; not a power of two
    first = vn.Model(**p).bins(frames[0])
    assert (vn.Model(**p).bins(frames[3:]) != first).all() and (vn.Model(**p).bins(frames[:3]) == first).all()
    rr, cc = np.indices(first.shape)
    tiny = np.finfo(np.float32).tiny
    den, zero = [], []

    def watch(t, m):
        v = m.hist[first, rr, cc]
        if ((v > 0) & (v < tiny)).all():
            den.append(t)
        if (v == 0).all():
            zero.append(t)

    m = run_restatement("denormal", watch)[0]
    assert den == list(range(DENORMAL_FIRST, DENORMAL_LAST + 1)) and zero == list(range(ZERO_FROM, len(frames)))
    assert (r["hist"][first, rr, cc] == 0).all() and m.denormal_seen == len(den) * first.size
    # denormal_mid is the same clip cut off inside the denormal stretch: its stored planes hold the denormals themselves, so an
    # engine that flushed them to zero could not reproduce the fixture
    r2, p2, frames2 = golden("denormal_mid")
    assert p2 == p and np.array_equal(frames2, frames[:len(frames2)]) and DENORMAL_FIRST < len(frames2) - 1 < DENORMAL_LAST
    v = r2["hist"][first, rr, cc]
    assert ((v > 0) & (v < tiny)).all()
    # products round inside the denormal range: the float product differs from the exactly scaled value there
    v = np.float32(1e-42)
    assert float(v * np.float32(p["alpha"])) != float(v) * float(np.float32(p["alpha"]))


def test_above_one_half_an_abandoned_bin_never_reaches_zero():
    """alpha >= 0.5 (the default 0.995 included): the smallest denormal times alpha rounds back to itself, so a bin that was hit
    once stays a non-zero denormal for ever.  This is what a flush-to-zero build would get wrong, and why the live-bin bitmap only
    ever shrinks for alpha < 0.5."""
    sub = np.float32(1.401298464324817e-45)
    for alpha in (0.995, 0.7, 0.51):
        assert sub * np.float32(alpha) == sub
    assert sub * np.float32(0.5) == 0 and sub * np.float32(0.49) == 0
    h = np.float32(0.005)
    for _ in range(30000):
        h = h * np.float32(0.995)
    assert 0 < h < np.finfo(np.float32).tiny and h * np.float32(0.995) == h


def test_scale_works_in_float_not_in_double():
    """cvConvertScale on 32F: fl32(h * (float)alpha).  The double product rounded once differs for a share of inputs."""
    h = np.random.RandomState(1).rand(100000).astype(np.float32)
    a = 0.995
    assert 0.01 < np.mean((h * np.float32(a)) != (h.astype(np.float64) * a).astype(np.float32)) < 0.9


def test_gray_formula():
    px = lambda b, g, r: int(vn.gray_rgb(np.array([[[b, g, r]]], np.uint8))[0, 0])  # noqa: E731
    assert px(255, 0, 0) == 76 and px(0, 0, 255) == 29 and px(0, 255, 0) == 150
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(vn.gray_rgb(np.stack([v, v, v], -1)[None]), v[None])


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------

def test_ids_and_struct_tail_match_c(tmp_path):
    inc = os.path.join(HERE, os.pardir, "include")
    src = tmp_path / "vu_sz.c"
    fields = ", ".join("offsetof(bgs_params, %s)" % f for f in VU_FIELDS)
    known = ", ".join("BGS_ALGO_KNOWN(%d)" % i for i in (-1, 0, 25, 26, 27, 28, 99))
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bgs_hip.h"\nint main(){printf("%zu %d %d %d %d %zu' + " %zu" * len(VU_FIELDS) + " %d" * 7
                   + '\\n", sizeof(bgs_params), (int)BGS_ALGO_COUNT, (int)BGS_ALGO_END, (int)BGS_VUMETER, (int)BGS_ALGO_LIMIT, '
                   "offsetof(bgs_params, lb_training_steps), " + fields + ", " + known + ");return 0;}\n")
    exe = tmp_path / "vu_sz"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(exe)], check=True)
    v = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert v[0] == C.sizeof(capi.BgsParams)
    assert v[1:5] == [21, 26, 27, 28] and capi.VUMETER == 27 and capi.ALGO_LIMIT == 28
    offs = v[6:10]
    assert offs == [getattr(capi.BgsParams, f).offset for f in VU_FIELDS]
    assert offs == sorted(offs) and offs[0] > v[5] == capi.BgsParams.lb_training_steps.offset  # grown at the end only
    assert v[10:] == [0, 1, 1, 0, 1, 0, 0]
    assert capi.BgsParams._fields_[-4:] == [("vu_bin_size", C.c_int32), ("vu_enable_filter", C.c_int32), ("vu_alpha", C.c_double), ("vu_threshold", C.c_double)]


def test_ids_26_and_28_are_invalid_and_27_is_valid():
    p = capi.BgsParams()
    p.struct_size = C.sizeof(capi.BgsParams)
    for bad in (26, 28, 99, -1):
        assert capi.lib().bgs_default_params(bad, C.byref(p)) == capi.ERR_INVALID, bad
        h = C.c_void_p()
        assert capi.lib().bgs_create(bad, None, 0, 1, C.byref(h)) == capi.ERR_INVALID and b"unknown algorithm" in capi.lib().bgs_last_error()
    assert capi.lib().bgs_default_params(27, C.byref(p)) == capi.OK
    for src in ("bgs_hip.hip", "bgs_node.cpp"):  # the three range checks go through the one helper
        text = open(os.path.join(HERE, os.pardir, "tracking_amd", "csrc", src)).read()
        assert "BGS_ALGO_KNOWN(algo)" in text and ">= BGS_ALGO_END" not in text and ">= BGS_ALGO_COUNT" not in text, src


def test_default_params():
    p = capi.default_params(capi.VUMETER)
    assert tuple(getattr(p, f) for f in VU_FIELDS) == (8, 1, 0.995, 0.03)
    assert (p.vu_bin_size, p.vu_alpha, p.vu_threshold, p.vu_enable_filter) == tuple(vn.DEFAULTS[k] for k in ("bin_size", "alpha", "threshold", "enable_filter"))
    for algo in range(26):
        q = capi.default_params(algo)
        assert all(getattr(q, f) == 0 for f in VU_FIELDS), algo


@pytest.mark.parametrize("field,value", [("vu_bin_size", 0), ("vu_bin_size", -3), ("vu_bin_size", 255), ("vu_bin_size", 1000), ("vu_alpha", 0.0), ("vu_alpha", 1.0),
                                         ("vu_alpha", 1.5), ("vu_alpha", -0.1), ("vu_threshold", 0.0), ("vu_threshold", 1.0), ("vu_threshold", 7.0)])
def test_out_of_range_values_are_replaced_not_refused(field, value):
    """The setters' rules (TBackgroundVuMeter.h:47-54) in the restatement, and bgs_create accepts the value (it fails only later, for
    want of a GPU, or not at all)."""
    kw = {field[3:]: value}
    m = vn.Model(**kw)
    assert (m.bin_size, m.alpha, m.threshold) == (8, 0.995, 0.03)
    assert vn.setters(254, 0.999, 0.999) == (254, 0.999, 0.999) and vn.setters(1, 1e-9, 1e-9) == (1, 1e-9, 1e-9)
    p = capi.default_params(capi.VUMETER)
    setattr(p, field, value)
    h = C.c_void_p()
    rc = capi.lib().bgs_create(capi.VUMETER, C.byref(p), 0, 1, C.byref(h))
    assert rc in (capi.OK, capi.ERR_HIP), capi.last_error()
    if rc == capi.OK:
        capi.lib().bgs_destroy(h)


# ---- host layer ------------------------------------------------------------------------------------------------------------------------

def test_reference_side_adapters_compile_with_vumeter(tmp_path):
    root = os.path.dirname(HERE)
    tu = tmp_path / "adapters_vu.cpp"
    tu.write_text('#include "HipBGS.h"\n#include "HipFGDetector.h"\nIBGS* make() { return new hipbgs::VuMeter; }\nCvFGDetector* make_fg() { return new HipFGDetector(31); }\n')
    r = subprocess.run(["g++", "-std=gnu++0x", "-fsyntax-only", "-Wall", "-I" + os.path.join(root, "tests", "mock_opencv"), "-I" + os.path.join(root, "include"),
                        "-I" + os.path.join(root, "tracking_amd", "host"), str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
